"""The fp64 reference of the top-n alternatives (tests/top_logprobs_ref.py) against torch, the crafted rows of the GPU tests against what
they claim to contain, and the host-side refusals - all without a GPU or the library."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import logprob_ref as L
import top_logprobs_ref as R

BF16 = torch.bfloat16


def _tie_free_rows(M, V, seed):
    """distinct bf16 values per row: a permutation of k / 8, |k| < 256 (exact in bf16)"""
    assert V <= 511
    g = torch.Generator().manual_seed(seed)
    grid = (torch.arange(-255, 256, dtype=torch.float32) / 8.0)
    return torch.stack([grid[torch.randperm(511, generator=g)[:V]] for _ in range(M)]).to(BF16)


@pytest.mark.parametrize("temp", [0.0, 2.0])          # a division by 2 is exact: the rows stay tie-free
@pytest.mark.parametrize("n", [1, 5, 20])
def test_reference_equals_torch_topk(n, temp):
    logits = _tie_free_rows(6, 330, 3)
    y = L.y_values(logits, temp)
    assert all(len(set(r.tolist())) == r.numel() for r in y)
    want_lp, want_ids = torch.topk(torch.log_softmax(y.double(), -1), n, dim=-1)
    fed = torch.tensor([0, 329, 17, 400, -1, 5])
    ids, lps, rank = R.top(logits, n, temp, fed)
    assert torch.equal(ids, want_ids)
    assert (lps - want_lp).abs().max() <= 1e-12
    full = torch.argsort(-y, dim=-1)
    for m, f in enumerate(fed.tolist()):
        want = 1 + int((full[m] == f).nonzero()[0]) if 0 <= f < 330 else 0
        assert int(rank[m]) == want


def test_reference_special_rows():
    row = torch.tensor([1.0, float("nan"), 2.0, 0.5], dtype=BF16)
    ok = torch.tensor([1.0, float("-inf"), 2.0, 2.0], dtype=BF16)
    ids, lps, rank = R.top(torch.stack([row, ok]), 3, 0.0, [2, 1])
    assert ids[0].tolist() == [-1, -1, -1] and torch.isnan(lps[0]).all() and int(rank[0]) == 0
    assert ids[1].tolist() == [2, 3, 0] and int(rank[1]) == 4
    assert float(lps[1, 0]) == float(lps[1, 1])
    ids, lps, rank = R.top(ok[None], 4, 0.0, [3])
    assert ids[0].tolist() == [2, 3, 0, 1] and lps[0, 3] == float("-inf") and int(rank[0]) == 2
    # one temperature per row
    both = torch.stack([R.row_collision(), R.row_collision()])
    a = R.top(both, 5, [0.0, R.T_COLLISION], [20, 20])
    assert a[0][0].tolist() == [5, 20, 200, 10, 40] and a[0][1].tolist() == [5, 10, 20, 40, 200]
    assert a[2].tolist() == [2, 3]


def test_crafted_rows_contain_what_they_claim():
    # the T = 1.5 row: inside its top n, two distinct logits with one y whose logit order is the reverse of the column order
    r = R.row_collision()
    n = 5
    y = L.y_values(r[None], R.T_COLLISION)[0]
    ids = R.top(r[None], n, R.T_COLLISION)[0][0].tolist()
    pairs = [(a, b) for a in ids for b in ids if a < b and y[a] == y[b] and float(r[a]) < float(r[b])]
    assert pairs, "no colliding pair inside the top n"
    assert (10, 20) in pairs and float(y[10]) == 2.015625
    assert ids.index(10) < ids.index(20)
    # the straddling row: the n-th value is shared across at least 3 tiles, by more columns than the top n has room for
    r = R.row_straddle()
    y = L.y_values(r[None])[0].numpy()
    order = np.argsort(-y, kind="stable")
    v = y[order[R.STRADDLE_N - 1]]
    tied = np.nonzero(y == v)[0]
    above = int((y > v).sum())
    assert len({int(c) // 16 for c in tied}) >= 3 and above < R.STRADDLE_N < above + len(tied)
    assert tuple(tied) == R.STRADDLE_TIED and order[:R.STRADDLE_N].tolist() == [17, 2048, 3001, 3500, 3999]
    # the tied columns sit where a sweep of 512 threads over 8-column chunks arrives last: chunks >= 375 of 514, two of them in the second pass
    assert min(tied) // 8 >= 375 and sum(1 for c in tied if c // 8 >= 512) >= 2
    # the others
    z = R.row_zeros_on_top()
    assert R.top(z[None], 3)[0][0].tolist() == [3, 7, 100] and (z.view(torch.int16)[[7, 100]] == -32768).all() and z.view(torch.int16)[3] == 0
    m = R.row_minus_inf()
    ids, lps, _ = R.top(m[None], 20)
    assert int(torch.isinf(m.float()).sum()) == 30 and torch.isfinite(lps[0, :10]).all() and (lps[0, 10:] == float("-inf")).all()
    assert ids[0, 10:].tolist() == sorted(ids[0, 10:].tolist()) == [c for c in range(40) if m[c] == float("-inf")][:10]
    last = R.row_max_in_last_column()
    assert R.top(last[None], 1)[0][0].tolist() == [329] and 329 % 16 != 15
    e = R.row_all_equal(4112)
    assert R.top(e[None], 20)[0][0].tolist() == list(range(20))
    f = R.row_forced()
    assert R.top(f[None], 1, 0.0, [50])[2].tolist() == [1]
    assert [int(R.top(f[None], 1, 0.0, [c])[2][0]) for c in (60, 61, 300, 7, 100, 330)] == [2, 3, 4, 329, 330, 0]


def test_host_refusals():
    """n outside 1..20, or above the vocabulary, is refused on the host: no library, no GPU"""
    from unimedvl_amd import _lib, ops
    from unimedvl_amd.decode import DecodeSession
    assert ops.check_top_logprobs(0) == 0 and ops.check_top_logprobs(20, 20) == 20
    for bad in (-1, 21, 2.5, True):
        with pytest.raises(ValueError, match="top_logprobs"):
            ops.check_top_logprobs(bad)
    with pytest.raises(ValueError, match="vocabulary"):
        ops.check_top_logprobs(11, 10)
    logits = torch.zeros((2, 12), dtype=BF16)
    ids = torch.zeros(2, dtype=torch.int64)
    for bad in (0, 21, 13):
        with pytest.raises(_lib.UmvError, match="n must be"):
            ops.top_logprobs(logits, ids, bad)
    llm = SimpleNamespace(cfg=SimpleNamespace(vocab=12))
    for bad in (21, 13, -1):
        with pytest.raises(ValueError, match="top_logprobs"):
            DecodeSession(llm, None, None, None, 4, top_logprobs=bad)
