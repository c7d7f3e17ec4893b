"""The numpy restatement of column MI for any alphabet size (tests/mica_wide_reference.py), pinned to the oracle where the
oracle is defined (up to 31 states).  Measured against the oracle on such inputs: 3.5e-14 (mi), 7.5e-14 (hjoint), 1.3e-15
(entropies); the bound leaves an order of magnitude."""
import numpy as np
import pytest

import oracle
import mica_wide_reference as ref


@pytest.mark.parametrize("T", [1, 33, 40, 65, 256])
@pytest.mark.parametrize("A", [2, 4, 5, 20, 21, 31])
def test_restatement_matches_the_oracle(A, T):
    a1 = ref.columns(A, T, 9, 100 * A + T, clean_half=False)
    a2 = ref.columns(A, T, 7, 100 * A + T + 1, clean_half=False)
    assert (a1[:, 1] >= A).all() and (a1[:, -1] == A - 1).all()
    if T >= 33:
        assert (a1 == A).any() and (a1 == 200).any()
    r, o = ref.mi_columns(a1, a2, A), oracle.mi_columns(a1, a2, A)
    for k in ("mi", "hjoint", "h1", "h2"):
        assert np.abs(r[k] - o[k]).max() <= 1e-12, (k, np.abs(r[k] - o[k]).max())
    ri = ref.mi_columns(a1, None, A)
    oi = oracle.mi_columns(a1, a1, A)
    for k in ("mi", "hjoint", "h1"):
        assert np.abs(ri[k] - oi[k]).max() <= 1e-12, k
    assert abs(r["h1"][1] - np.log(A)) <= 1e-12 and r["h1"][-1] == 0.0
    assert np.abs(r["mi"][1]).max() <= 1e-12 and np.abs(r["mi"][-1]).max() <= 1e-12
    p = ref.mi_pairs(a1, [0, 3, 3, 1], [2, 3, 6, 1], A, a2)
    assert np.abs(p["mi"] - r["mi"][[0, 3, 3, 1], [2, 3, 6, 1]]).max() <= 1e-12


def test_information_identity_at_64_states():
    """mi = h1 + h2 - hjoint holds with unknowns too: the margins of the spread joint table are the columns' own"""
    a = ref.columns(64, 256, 40, 9)
    assert (a == 63).any() and (a >= 64).any()
    r = ref.mi_columns(a, None, 64)
    assert np.abs(r["mi"] - (r["h1"][:, None] + r["h2"][None, :] - r["hjoint"])).max() <= 1e-12
