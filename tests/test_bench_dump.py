"""bench.py --dump-outputs (host side, no GPU): every --pair-output form is written as float64 .npy files, the sampled
entries are the ones named by pair_i / pair_j, null_pos and counts_sites, and the same inputs give the same files."""
import os
import types

import numpy as np
import pytest
import torch

import bench
from comap_amd import engine as E
from comap_amd.pipeline import sum_pairs


def _analysis(n, rows, n_null, seed=0):
    g = torch.Generator().manual_seed(seed)
    f64 = lambda *s: torch.rand(*s, dtype=torch.float64, generator=g)
    a = types.SimpleNamespace(n=n, aln=torch.zeros(1, n, dtype=torch.uint8), norm=f64(n), post_rate=f64(n), logL=f64(n),
                              rate_class=torch.randint(0, 10, (n,), dtype=torch.int32, generator=g), counts=f64(rows, n),
                              stat=f64(n, n), pvalue=f64(n, n), nsim=torch.randint(0, 99, (n, n), dtype=torch.int32, generator=g))
    null = dict(stat=f64(n_null), nmin=f64(n_null))
    a.null_buffers = lambda m: null
    return a


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


@pytest.mark.parametrize("n, rb, re_", [(300, 0, 300), (300, 17, 211), (700, 650, 700)])
def test_compact_records_are_sampled_with_their_pairs(tmp_path, monkeypatch, n, rb, re_):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 4096)
    a = _analysis(n, 126, 5000)
    ij = np.array([(i, j) for i in range(rb, re_) for j in range(i + 1, n)])
    rec = np.zeros(sum_pairs(n, rb, re_), dtype=E.PAIR_COMPACT)
    rec["stat"], rec["below"], rec["nsim"] = ij[:, 0] * 1e4 + ij[:, 1], ij[:, 0], ij[:, 1]
    for d in (tmp_path / "a", tmp_path / "b"):
        bench.dump_outputs(str(d), a, (torch.from_numpy(rec.view(np.uint8).copy()), len(rec)), "compact", rb, re_, 5000)
    got, again = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert got.keys() == again.keys() and all(np.array_equal(got[k], again[k]) for k in got)
    assert all(v.dtype == np.float64 for v in got.values())
    pi, pj = got["pair_i"], got["pair_j"]
    assert len(pi) == min(len(rec), 4096) and (np.diff(pi * n + pj) > 0).all()
    assert np.array_equal(got["pair_stat"], pi * 1e4 + pj) and np.array_equal(got["pair_below"], pi)
    assert np.array_equal(got["pair_nsim"], pj)
    assert np.array_equal(got["null_stat"], a.null_buffers(0)["stat"].numpy()[got["null_pos"].astype(int)])
    assert np.array_equal(got["counts"], a.counts.numpy()[:, got["counts_sites"].astype(int)])
    assert np.array_equal(got["rate_class"], a.rate_class.numpy())


def test_rows_and_dense_forms(tmp_path):
    a = _analysis(300, 30, 0)
    rows = np.zeros(1000, dtype=E.PAIR_ROW)
    rows["i"], rows["pvalue"] = np.arange(1000), np.arange(1000) * 0.5
    bench.dump_outputs(str(tmp_path / "rows"), a, (torch.from_numpy(rows.view(np.uint8).copy()), torch.tensor([700])),
                       "rows", 0, 300, 0)
    got = _load(tmp_path / "rows")
    assert "null_stat" not in got and len(got["pair_i"]) == 700
    assert np.array_equal(got["pair_pvalue"], got["pair_i"] * 0.5)
    bench.dump_outputs(str(tmp_path / "dense"), a, None, "dense", 0, 300, 0)
    got = _load(tmp_path / "dense")
    i, j = got["pair_i"].astype(int), got["pair_j"].astype(int)
    assert len(i) == 300 * 300 and np.array_equal(got["pair_stat"], a.stat.numpy()[i, j])
    assert np.array_equal(got["pair_nsim"], a.nsim.numpy()[i, j])

