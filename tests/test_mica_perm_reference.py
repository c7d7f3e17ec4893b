"""The numpy / Python restatement of Mica's permutation test for any alphabet (tests/mica_perm_reference.py) is the
yardstick of tests/test_gpu_mica_perm_wide.py; here it is pinned, as bytes, to the oracle where the oracle is generic (up to
31 states: 32-bit masks, 32 extended codes).  No GPU."""
import numpy as np
import pytest

import oracle
import mica_perm_reference as ref
import mica_wide_reference as wide

SHAPES = [(2, 33, 8), (7, 30, 10), (20, 41, 8), (31, 40, 10), (4, 2, 5)]


@pytest.mark.parametrize("A,T,n", SHAPES)
def test_the_restatement_equals_the_oracle(A, T, n):
    aln = wide.columns(A, T, n, 1000 * A + T)
    assert (aln >= A).any()
    pv, nb, gen = ref.permutation_test(aln, A, 130, 41)
    opv, onb = oracle.mica_permutation_test(aln, A, 130, 41)
    assert pv.tobytes() == opv.tobytes() and nb.tobytes() == onb.tobytes()
    if n >= 8:
        assert gen.any() and not gen.all() and (nb == 0).any() and (nb > 0).any()   # both paths, constant pairs and tested ones


def test_the_inputs_of_the_device_tests_too():
    A, T, n = 7, 30, 14
    aln = ref.columns(A, T, n, 1000 * A + T)
    pv, nb, gen = ref.permutation_test(aln, A, 200, 41)
    opv, onb = oracle.mica_permutation_test(aln, A, 200, 41)
    assert pv.tobytes() == opv.tobytes() and nb.tobytes() == onb.tobytes()
    assert (aln[:, 1] >= A).all() and (aln[:, n - 2] == A - 1).all() and (aln[:, n - 1] >= A).sum() == 1
    assert (nb[[0]] == 0).all() and gen[0]                       # pair (0, 1): an all-unknown column is constant


def test_a_pair_range_is_a_slice_of_the_full_result():
    A, T, n = 31, 40, 10
    aln = wide.columns(A, T, n, 1000 * A + T)
    pv, nb, gen = ref.permutation_test(aln, A, 130, 41)
    rpv, rnb, rgen = ref.permutation_test(aln, A, 130, 41, 7, 31)
    assert rpv.tobytes() == pv[7:31].tobytes() and rnb.tobytes() == nb[7:31].tobytes() and (rgen == gen[7:31]).all()
    opv, onb = oracle.mica_permutation_test(aln, A, 130, 41, 7, 31)
    assert rpv.tobytes() == opv.tobytes() and rnb.tobytes() == onb.tobytes()
