"""fp64 restatement of the top-n alternative tokens and token ranks (include/unimedvl_hip.h, "top-n alternative tokens and token
ranks") for the tests, and the crafted rows both test files use.

    y[c]            as the token log-probabilities define it (logprob_ref.y_values); -0 == +0
    order           the columns by (y descending, column ascending): a STABLE sort of -y
    top_ids[j]      the j-th column of that order, j < n
    top_logprobs[j] y[top_ids[j]] - logsumexp y            (logprob_ref.logsumexp)
    rank            1 + the number of columns in front of the fed token, by counting; 0 for a token outside [0, V)
    a row with a NaN: ids -1, log-probabilities NaN, rank 0

Everything after y is float64 / integer on the CPU.  Nothing here shares code with the kernels.
"""
import numpy as np
import torch

import logprob_ref as L

BF16 = torch.bfloat16


def top(logits, n, temperature=0.0, fed=None):
    """[M, V] bf16 logits -> (ids int64 [M, n], logprobs float64 [M, n], rank int64 [M]).  temperature: one value or one per row;
    fed: [M] tokens whose rank is wanted (None: rank 0 everywhere)."""
    M, V = logits.shape
    temps = [float(temperature)] * M if np.isscalar(temperature) else [float(t) for t in temperature]
    ids = np.full((M, n), -1, dtype=np.int64)
    lps = np.full((M, n), np.nan, dtype=np.float64)
    rank = np.zeros(M, dtype=np.int64)
    cols = np.arange(V)
    for m in range(M):
        y_t = L.y_values(logits[m:m + 1], temps[m])
        y = y_t[0].numpy() + 0.0                         # -0 -> +0
        if np.isnan(y).any():
            continue
        lse = float(L.logsumexp(y_t)[0])
        order = np.argsort(-y, kind="stable")
        ids[m] = order[:n]
        with np.errstate(invalid="ignore"):
            lps[m] = y[order[:n]] - lse
        f = -1 if fed is None else int(fed[m])
        if 0 <= f < V:
            rank[m] = 1 + int((y > y[f]).sum()) + int(((y == y[f]) & (cols < f)).sum())
    return torch.from_numpy(ids), torch.from_numpy(lps), torch.from_numpy(rank)


def logprobs_close(got, want, bound):
    """the largest |got - want| over the finite entries of want, after asserting that the others (-inf, NaN) agree exactly"""
    got, want = got.double().cpu(), want.double().cpu()
    fin = torch.isfinite(want)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), "NaN entries differ"
    inf = torch.isinf(want)
    assert torch.equal(got[inf], want[inf]), "infinite entries differ"
    return float((got[fin] - want[fin]).abs().max()) if fin.any() else 0.0


# ----------------------------------------------------------------------------- crafted rows
# every builder returns one bf16 row [V]; what the row is for is asserted in test_top_logprobs_cpu.py
T_COLLISION = 1.5
COLLISION_LO, COLLISION_HI = 3.015625, 3.03125      # both give bf16(x / 1.5) = 2.015625
STRADDLE_V, STRADDLE_N = 4112, 5
STRADDLE_TIED = (3001, 3500, 3999, 4090, 4097, 4105, 4111)    # one shared value, in seven tiles, the last ones of the row


def _background(V, seed, hi=-1.0):
    """distinct-ish values well below `hi`"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(V, generator=g) * 4.0 - 6.0 + (hi + 1.0)).to(BF16)


def row_all_equal(V, value=1.5):
    return torch.full((V,), value, dtype=BF16)


def row_straddle():
    """two values above, then the n-th value (2.0) shared by STRADDLE_TIED: the class must give its three lowest columns, and those sit
    where a thread-strided sweep arrives last - the highest threads of the first pass and the chunks of the second"""
    r = _background(STRADDLE_V, 11)
    r[17], r[2048] = 5.0, 4.0
    for c in STRADDLE_TIED:
        r[c] = 2.0
    return r


def row_zeros_on_top(V=330):
    r = _background(V, 12)
    r[7], r[3], r[100] = -0.0, 0.0, -0.0
    return r


def row_minus_inf(V=40):
    """30 columns of -inf, 10 finite ones"""
    r = torch.full((V,), float("-inf"), dtype=BF16)
    finite = [1, 4, 9, 16, 17, 25, 31, 32, 36, 39]
    r[finite] = _background(len(finite), 13)
    return r


def row_max_in_last_column(V=330):
    r = _background(V, 14)
    r[V - 1] = 3.0
    return r


def row_collision(V=330):
    """two pairs of distinct logits that share one y at T = 1.5, the smaller logit in the lower column"""
    r = _background(V, 15)
    r[10], r[20] = COLLISION_LO, COLLISION_HI
    r[200], r[40] = COLLISION_HI, COLLISION_LO
    r[5] = 6.0
    return r


def row_forced(V=330):
    """columns with known ranks: 50 the maximum; 60, 61, 300 tied behind it; 7 and 100 are -inf"""
    r = _background(V, 16)
    r[50] = 4.0
    r[60] = r[61] = r[300] = 3.0
    r[7] = r[100] = float("-inf")
    return r
