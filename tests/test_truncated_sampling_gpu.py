"""Truncated sampling (top-k / top-p / min-p; include/unimedvl_hip.h, "truncated sampling") on the GPU: the stand-alone entry and the
step-end entry against the fp64 reference of the definition (tests/truncation_ref.py), against the lm_head sampling epilogue whose
noise they share, and through the engine.

Bounds.  top-k works on integer counts: n_kept and cut_y are asserted EXACTLY.  top-p and min-p are asserted by the band rule with
EPS = 2e-6: expf is within 2 ulp (2.4e-7 relative) of exp, the sums are fp64, doubled for the ratio of two such sums and rounded up;
the device's cutoff class c must leave a mass fraction >= top_p - EPS at or above c and < top_p + EPS strictly above it, must keep every
class with y - M >= ln(min_p) + EPS and drop every class with y - M <= ln(min_p) - EPS.  No row is left out.  Every test prints the
largest deviation it saw before it asserts (`pytest -s`); on an MI355X every cutoff was the definition's own class (deviation 0).
Frequencies: chi2 < dof + 6 sqrt(2 dof) over the cells with expectation > 5, the bound of the existing sampler tests."""
import functools
import math

import numpy as np
import pytest
import torch

import logprob_ref as LR
import truncation_ref as R
from conftest import NEW_TOKEN_IDS

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
EPS = 2e-6
T = 0.7
SEED = 4321
BOUND = 1e-4          # of a log-probability: the bound test_logprob_gpu.py derives
COMBINED = dict(top_k=50, top_p=0.9, min_p=0.05)


def _ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _logits(rows, V, kind="normal"):
    """bf16 logits [rows, V] on the host.  normal: N(0, 2^2); grid: a 0.5 grid, so that most classes hold several columns and ties
    straddle every k; the last row of a many-row case is peaked (one logit 12 above the rest)."""
    g = torch.Generator().manual_seed(1000 * rows + V + len(kind))
    x = torch.randn(rows, V, generator=g) * 2
    if kind == "grid":
        x = (x * 2).round() / 2
    if rows > 1:
        x[-1, V // 3] = x[-1].max() + 12
    return x.to(BF16)


@functools.lru_cache(maxsize=None)
def _rows(rows, V, kind, temp):
    """the reference's classes of every row, computed once"""
    y = R.pick_value(_logits(rows, V, kind), temp)
    return y, [R.classes(y[r]) for r in range(rows)]


def _draw(logits_dev, temp, step=0, seed=SEED, **flt):
    ops = _ops()
    M = logits_dev.shape[0]
    cut = torch.full((M,), 77.0, dtype=torch.float32, device="cuda")
    kept = torch.full((M,), -3, dtype=torch.int32, device="cuda")
    st = torch.full((1,), step, dtype=torch.int64, device="cuda")
    ids = ops.sample_truncated(logits_dev, temp, seed, step=st, cut_y=cut, n_kept=kept, **flt)
    return ids.cpu(), cut.cpu(), kept.cpu()


def _check(y, rows, ids, cut, kept, flt, exact=False):
    """every row: the device's cutoff is a class of the row inside the band (the definition's own class where exact), n_kept is the
    column count down to it, the drawn id lies at or above it.  Returns the largest deviation (truncation_ref.deviation)."""
    worst = 0.0
    for r, row in enumerate(rows):
        c = float(cut[r])
        i = row.index_of(c)
        assert i is not None, f"row {r}: cut_y {c} is no class of the row"
        lo, hi = R.band(row, eps=EPS, **flt)
        want = R.cutoff(row, **flt)
        if exact:
            assert (i, int(kept[r])) == (want[0], want[2]), f"row {r}: class {i} n_kept {int(kept[r])}, reference {want}"
        assert lo <= i <= hi, f"row {r}: class {i} outside the band [{lo}, {hi}] (reference {want[0]})"
        assert int(kept[r]) == int(row.cumcnt[i]), f"row {r}: n_kept {int(kept[r])} != {int(row.cumcnt[i])} columns down to class {i}"
        t = int(ids[r])
        assert 0 <= t < y.shape[1]
        yt = float(y[r, t])
        assert (math.isnan(c) and math.isnan(yt)) or yt >= c, f"row {r}: drew column {t} with y {yt} below the cutoff {c}"
        worst = max(worst, R.deviation(row, i, **flt))
    return worst


# ----------------------------------------------------------------------------- 1-4. the cutoff and the draw, against the definition
@pytest.mark.parametrize("rows", [1, 8, 64])
@pytest.mark.parametrize("V", [40, 70, 320, 4112])
def test_cutoff_and_draw_follow_the_definition(V, rows):
    worst = 0.0
    for kind in ("normal", "grid"):
        dev = _logits(rows, V, kind).cuda()
        y, ref = _rows(rows, V, kind, T)
        for k in (1, 4, 50, V, V + 7):                                       # top-k alone: exact, tied rows included
            flt = dict(top_k=k)
            _check(y, ref, *_draw(dev, T, **flt), flt, exact=True)
        for flt in (dict(top_p=0.9), dict(top_p=0.3), dict(min_p=0.05), dict(min_p=0.5), COMBINED, dict(top_k=4, top_p=0.5)):
            worst = max(worst, _check(y, ref, *_draw(dev, T, **flt), flt))
    print(f"V={V} rows={rows}: largest deviation from the definition's cutoff {worst:.3g}")
    assert worst <= EPS


def test_full_vocabulary():
    """2 rows at V = 152 064: N(0, 2^2) logits and a peaked row; an odd row stride too (no 16-byte loads)"""
    V = 152064
    dev = _logits(2, V).cuda()
    y, ref = _rows(2, V, "normal", T)
    worst = 0.0
    for flt, exact in ((dict(top_k=50), True), (dict(top_k=1), True), (dict(top_p=0.9), False), (dict(min_p=0.05), False), (COMBINED, False)):
        got = _draw(dev, T, **flt)
        worst = max(worst, _check(y, ref, *got, flt, exact=exact))
        wide = torch.zeros((2, V + 3), dtype=BF16, device="cuda")
        wide[:, :V] = dev
        again = _draw(wide[:, :V], T, **flt)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), "the row stride changed the result"
    print(f"V={V}: largest deviation {worst:.3g}")
    assert worst <= EPS


# ----------------------------------------------------------------------------- 5. equality against the lm_head sampling epilogue
def _step_bufs(B, max_len, s=0):
    dev = "cuda"
    return dict(slot=torch.arange(10, 10 + B, dtype=torch.int32, device=dev), pos=torch.arange(20, 20 + B, dtype=torch.int32, device=dev),
                kvl=torch.arange(11, 11 + B, dtype=torch.int32, device=dev), ids=torch.full((B,), -5, dtype=torch.int64, device=dev),
                in_ids=torch.full((max_len, B), -7, dtype=torch.int64, device=dev),
                pred=torch.full((max_len, B), -9, dtype=torch.int64, device=dev),
                step=torch.full((B,), s, dtype=torch.int64, device=dev),
                lp=torch.full((max_len, B), 99.0, dtype=torch.float32, device=dev),
                cut=torch.full((max_len, B), 77.0, dtype=torch.float32, device=dev),
                kept=torch.full((max_len, B), -3, dtype=torch.int32, device=dev))


def _key_ids(keys):
    k = keys.cpu().numpy().view(np.uint64).max(axis=1)
    return torch.from_numpy((np.uint64(0xFFFFFFFF) - (k & np.uint64(0xFFFFFFFF))).astype(np.int64))


@pytest.mark.parametrize("V", [40, 320])
def test_equality_with_the_lm_head_sampling_epilogue(V):
    """x = e_0, so every row's logits are W[:, 0]; 64 rows, steps 0..7.  The yardstick is the epilogue's own Gumbel-max: with filters
    that keep everything the truncated entries must return its ids; with restrictive filters, its ids on a second weight whose dropped
    columns hold -1e30 - the argmax over the kept set under the same noise."""
    ops = _ops()
    K, rows = 32, 64
    g = torch.Generator().manual_seed(81 + V)
    w = torch.zeros((V, K))
    w[:, 0] = torch.randn(V, generator=g) * 2
    w = w.to(BF16)
    x = torch.zeros((rows, K), dtype=BF16, device="cuda")
    x[:, 0] = 1.0
    y = R.pick_value(w[:, 0], T)
    row = R.classes(y)
    lin = ops.PackedLinear.from_weight(w.cuda())
    nt = (V + 15) // 16
    for flt in (dict(top_k=V), dict(top_k=5, top_p=0.8), dict(top_p=0.6), dict(min_p=0.2)):
        i, cut_ref, n_ref = R.cutoff(row, **flt)
        w2 = w.clone()
        w2[y < cut_ref, 0] = -1e30
        lin2 = ops.PackedLinear.from_weight(w2.cuda())
        n_fast = n_slow = 0
        for s in range(8):
            b = _step_bufs(rows, 9, s)
            keys = torch.zeros((rows, nt), dtype=torch.int64, device="cuda")
            out = torch.empty((rows, V), dtype=BF16, device="cuda")
            ops.gemm(x, lin, out=out, argmax_partial=keys, sample=(T, SEED, b["step"]))
            fused = _key_ids(keys)                                                   # the untruncated pick
            keys2 = torch.zeros_like(keys)
            ops.gemm(x, lin2, out=torch.empty_like(out), argmax_partial=keys2, sample=(T, SEED, b["step"]))
            want = _key_ids(keys2)                                                   # the argmax over the kept set, same noise
            alone, cut, kept = _draw(out, T, step=s, **flt)
            assert (cut == cut_ref).all() and (kept == n_ref).all(), f"{flt}: the cutoff differs from the reference's"
            ops.decode_step_end_truncated(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"], out, T, SEED,
                                          cut_y=b["cut"], n_kept=b["kept"], **flt)
            end = b["ids"].cpu()
            assert torch.equal(alone, end), f"{flt} step {s}: stand-alone and step-end entries disagree"
            assert torch.equal(alone, want), f"{flt} step {s}: not the epilogue's pick over the kept set"
            if flt == dict(top_k=V):
                assert torch.equal(alone, fused)
            assert torch.equal(b["pred"][s].cpu(), end) and torch.equal(b["in_ids"][s + 1].cpu(), end)
            assert (b["cut"][s].cpu() == cut_ref).all() and (b["kept"][s].cpu() == n_ref).all()
            assert (b["step"] == s + 1).all() and (b["slot"].cpu() == torch.arange(11, 11 + rows)).all() and (b["lp"] == 99.0).all()
            stays = y[fused] >= cut_ref
            assert torch.equal(end[stays], fused[stays])
            n_fast += int(stays.sum())
            n_slow += int((~stays).sum())
        if flt != dict(top_k=V):
            assert n_fast > 0 and n_slow > 0, f"{flt}: both branches of the step-end kernel must be taken (kept {n_fast}, not kept {n_slow})"
        else:
            assert n_slow == 0


# ----------------------------------------------------------------------------- 6. the distribution
@pytest.mark.parametrize("flt", [dict(top_p=0.8), dict(top_k=5), dict(min_p=0.1)], ids=["top_p", "top_k", "min_p"])
def test_frequencies_follow_the_truncated_softmax(flt):
    V, rows = 40, 4096
    g = torch.Generator().manual_seed(81)
    one = (torch.randn(V, generator=g) * 0.7).to(BF16)         # flat enough that the three filters keep 12, 5 and 10 columns
    dev = one.expand(rows, V).contiguous().cuda()
    y = R.pick_value(one, T)
    row = R.classes(y)
    i, cut_ref, n_ref = R.cutoff(row, **flt)
    p = R.truncated_probs(row, y, i)
    assert 5 <= n_ref < V
    counts = torch.zeros(V, dtype=torch.float64)
    for seed in (11, 12, 13, 14):
        ids, cut, kept = _draw(dev, T, seed=seed, **flt)
        assert (cut == cut_ref).all() and (kept == n_ref).all()
        counts += torch.bincount(ids, minlength=V).double()
    assert counts[p == 0].sum() == 0, "a draw outside the kept set"
    exp = p * counts.sum()
    mask = exp > 5
    chi2 = (((counts - exp) ** 2) / exp)[mask].sum().item()
    dof = int(mask.sum()) - 1
    print(f"{flt}: chi2 {chi2:.1f} for {dof} dof, {n_ref} columns kept")
    assert chi2 < dof + 6 * (2 * dof) ** 0.5, f"chi2 {chi2:.1f} for {dof} dof"


# ----------------------------------------------------------------------------- 7. determinism and batch independence
@pytest.mark.parametrize("V", [70, 4112])
def test_determinism_and_batch_independence(V):
    dev = _logits(64, V).cuda()
    for flt in (COMBINED, dict(top_p=0.9)):
        a, b = _draw(dev, T, step=3, **flt), _draw(dev, T, step=3, **flt)
        assert all(torch.equal(u, v) for u, v in zip(a, b)), "the same call twice"
        few = _draw(dev[:8].contiguous(), T, step=3, **flt)
        assert all(torch.equal(u[:8], v) for u, v in zip(a, few)), "rows 0..7 of 64 against a call of 8 rows"
        c = _draw(dev, T, step=4, **flt)
        assert torch.equal(a[1], c[1]) and torch.equal(a[2], c[2]) and not torch.equal(a[0], c[0]), "another step: other draws, the same cutoff"


# ----------------------------------------------------------------------------- 8. edges
def test_edges():
    ops = _ops()
    V = 320
    x = _logits(8, V, "grid").clone()
    x[0, 5] = x[0, 200] = x[0].max()                      # a tied maximum
    x[1, 17] = float("nan")
    x[2] = float("-inf")
    x[3, :100] = float("-inf")
    x[4, 9] = float("inf")
    dev = x.cuda()
    y = R.pick_value(x, T)
    rows = [R.classes(y[r]) for r in range(8)]
    ids, cut, kept = _draw(dev, T, top_k=1)
    _check(y, rows, ids, cut, kept, dict(top_k=1), exact=True)
    for r in (0, 3, 4, 5, 6, 7):
        assert float(y[r, int(ids[r])]) == float(y[r].max()), f"row {r}: top_k = 1 picks a column of the maximal class"
    assert int(kept[0]) >= 2 and int(ids[0]) in (y[0] == y[0].max()).nonzero().flatten().tolist()
    for flt in (dict(top_k=1), dict(top_p=0.5), dict(min_p=0.3), COMBINED):
        ids, cut, kept = _draw(dev, T, **flt)
        assert int(ids[1]) == 17 and math.isnan(float(cut[1])) and int(kept[1]) == 1, "a NaN column wins"
        assert int(ids[4]) == 9 and float(cut[4]) == float("inf") and int(kept[4]) == 1, "a +inf column is the whole mass"
        _check(y, rows, ids, cut, kept, flt)
    everything = _draw(dev, T, top_k=V)
    for flt in (dict(top_k=3), dict(top_p=0.5), dict(min_p=0.3), COMBINED):
        got = _draw(dev, T, **flt)
        assert int(got[0][2]) == int(everything[0][2]) and float(got[1][2]) == float("-inf") and int(got[2][2]) == V, "a row of -inf only"
    assert all(int(everything[2][r]) == V for r in range(8) if r != 1)                  # (row 1: the NaN class takes all)
    with pytest.raises(Exception, match="no filter"):
        ops.sample_truncated(dev, T, SEED)
    for bad in (dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.01), dict(min_p=1.0), dict(min_p=-0.5)):
        with pytest.raises(Exception, match=next(iter(bad))):
            ops.sample_truncated(dev, T, SEED, **bad)
    with pytest.raises(Exception, match="temperature"):
        ops.sample_truncated(dev, 0.0, SEED, top_k=5)


def test_step_end_with_forced_tokens_and_logprobs():
    """the forced token is fed, pred_ids records the truncated pick, the log-probability is the forced token's UNTRUNCATED one"""
    ops = _ops()
    N, B, K, L = 1000, 5, 64, 3
    g = torch.Generator().manual_seed(6)
    lin = ops.PackedLinear.from_weight((torch.randn(N, K, generator=g) * 0.3).to(BF16).cuda())
    x = torch.randn(B, K, generator=g).to(BF16).cuda()
    nt = (N + 15) // 16
    forced = torch.full((L, B), -1, dtype=torch.int64)
    forced[:, 0] = torch.tensor([3, 999, 0])
    forced[1, 2] = 42
    forced = forced.cuda()
    b = _step_bufs(B, L)
    for s in range(L):
        keys = torch.zeros((B, nt), dtype=torch.int64, device="cuda")
        st = torch.zeros((B, nt, 2), dtype=torch.float32, device="cuda")
        out = torch.empty((B, N), dtype=BF16, device="cuda")
        ops.gemm(x, lin, out=out, argmax_partial=keys, lse_partial=st, sample=(T, SEED, b["step"]))
        pick, cut, kept = _draw(out, T, step=s, **COMBINED)
        ops.decode_step_end_truncated(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"], out, T, SEED,
                                      lse_partial=st, logprobs=b["lp"], forced_ids=forced, cut_y=b["cut"], n_kept=b["kept"], **COMBINED)
        fed = torch.where(forced[s].cpu() >= 0, forced[s].cpu(), pick)
        assert torch.equal(b["pred"][s].cpu(), pick) and torch.equal(b["ids"].cpu(), fed)
        if s + 1 < L:
            assert torch.equal(b["in_ids"][s + 1].cpu(), fed)
        assert torch.equal(b["cut"][s].cpu(), cut) and torch.equal(b["kept"][s].cpu(), kept)
        err = (b["lp"][s].double().cpu() - LR.logprob(out, fed.cuda(), T)).abs().max().item()
        print(f"step {s}: largest |logprob error| {err:.3g}")
        assert err <= 1e-4
    assert (b["step"] == L).all()


# ----------------------------------------------------------------------------- 8b. more tiles than one pass of the tile loops
V_MANY, PEAKS = 65560, (5, 16 * 2048 + 3, 65555)


@functools.lru_cache(maxsize=None)
def _many_tiles():
    """4098 tiles: two passes of the 512-thread step end's walk over the keys (8 loads in flight: 4096 tiles a pass) and nine of its
    walks over the statistics, the last of each partial.  x = e_r, so row r's logits are column r of the weight: N(0, 2^2) and one
    logit 30 above the row maximum at PEAKS[r] - in tile 0, in tile 2048, in the last tile (8 columns).  Sampled at step 0."""
    ops = _ops()
    K, B, nt = 32, len(PEAKS), (V_MANY + 15) // 16
    w = torch.zeros((V_MANY, K))
    w[:, :B] = torch.randn(V_MANY, B, generator=torch.Generator().manual_seed(V_MANY)) * 2
    for r, c in enumerate(PEAKS):
        w[c, r] = w[:, r].max() + 30
    x = torch.zeros((B, K), dtype=BF16, device="cuda")
    x[torch.arange(B), torch.arange(B)] = 1.0
    keys = torch.zeros((B, nt), dtype=torch.int64, device="cuda")
    st = torch.full((B, nt, 2), 7.0, dtype=torch.float32, device="cuda")
    out = torch.full((B, V_MANY), 3.0, dtype=BF16, device="cuda")
    ops.gemm(x, ops.PackedLinear.from_weight(w.to(BF16).cuda()), out=out, argmax_partial=keys, lse_partial=st,
             sample=(T, SEED, torch.zeros(B, dtype=torch.int64, device="cuda")))
    return out, keys, st


@pytest.mark.parametrize("with_logprobs", [False, True])
def test_more_tiles_than_one_pass(with_logprobs):
    ops = _ops()
    out, keys, st = _many_tiles()
    B = len(PEAKS)
    y = R.pick_value(out.cpu(), T)
    for flt in (dict(top_k=V_MANY), dict(top_k=1)):
        b = _step_bufs(B, 2)
        lp = dict(lse_partial=st, logprobs=b["lp"]) if with_logprobs else {}
        ops.decode_step_end_truncated(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"], out, T, SEED,
                                      cut_y=b["cut"], n_kept=b["kept"], **lp, **flt)
        ids = b["ids"].cpu()
        if flt["top_k"] == 1:
            assert ids.tolist() == list(PEAKS) and (b["kept"][0] == 1).all()
            assert torch.equal(b["cut"][0].cpu(), y[torch.arange(B), torch.tensor(PEAKS)].float())
        else:
            assert torch.equal(ids, _key_ids(keys)), "nothing dropped: the maximum over the keys"
        assert torch.equal(b["pred"][0].cpu(), ids) and torch.equal(b["in_ids"][1].cpu(), ids) and (b["step"] == 1).all()
        if with_logprobs:
            err = (b["lp"][0].double().cpu() - LR.logprob(out, b["ids"], T)).abs().max().item()
            print(f"{flt}: largest |logprob error| {err:.3g}")
            assert err <= BOUND and (b["lp"][1] == 99.0).all()
        else:
            assert (b["lp"] == 99.0).all()


# ----------------------------------------------------------------------------- the engine, at the tiny configuration
@pytest.fixture(scope="module")
def model(tiny_weights):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.config import UniMedVLConfig
    cfg, sd, _, _ = tiny_weights
    return Bagel(UniMedVLConfig.from_dict(cfg), lambda n: sd[n], device="cuda", visual_gen=False)


PROMPTS = [[11, 22, 33, 44, 55], [66, 77, 88], [99, 111, 122, 133]]
SAMPLE = dict(do_sample=True, temperature=T, seed=77)


def _session(model, steps=8, B=3, **kw):
    from unimedvl_amd.decode import DecodeSession
    from unimedvl_amd.kvcache import NaiveCache

    class Tok:
        def encode(self, s):
            return PROMPTS[int(s) % 3] + [int(s) // 3 + 5] * (int(s) // 3 > 0)
    cache = NaiveCache(model.cfg.layers)
    gi, kvl, rope = model.prepare_prompts([0] * B, [0] * B, [str(i) for i in range(B)], Tok(), NEW_TOKEN_IDS)
    cache = model.forward_cache_update_text(cache, **gi)
    gi = model.prepare_start_tokens(kvl, rope, NEW_TOKEN_IDS)
    with torch.no_grad():
        return DecodeSession(model.language_model, cache, gi["packed_start_tokens"], gi["packed_query_position_ids"], steps, **kw)


def test_filters_off_is_the_old_path(model):
    with torch.no_grad():
        old = _session(model, **SAMPLE)
        old.step(8)
        new = _session(model, top_k=0, top_p=1.0, min_p=0.0, **SAMPLE)
        new.step(8)
    assert torch.equal(old.pred_ids, new.pred_ids) and torch.equal(old.in_ids, new.in_ids)
    assert new.truncated is False and new.pred_cut_y is None and new.pred_n_kept is None and new.lse_part is None


def test_graph_replay_equals_eager(model):
    flt = dict(top_p=0.9, top_k=20)
    with torch.no_grad():
        g = _session(model, use_graph=True, **flt, **SAMPLE)
        assert g.graph is not None and g.pred_cut_y.shape == (8, 3) and g.pred_n_kept.dtype == torch.int32
        g.step(8)
        e = _session(model, use_graph=False, **flt, **SAMPLE)
        e.step(8)
    assert torch.equal(g.pred_ids, e.pred_ids) and torch.equal(g.in_ids, e.in_ids)
    assert torch.equal(g.pred_n_kept, e.pred_n_kept) and torch.equal(g.pred_cut_y, e.pred_cut_y)


@pytest.mark.parametrize("flt", [dict(top_p=0.9, top_k=20), dict(min_p=0.1), dict(top_p=0.5)], ids=["topk_topp", "min_p", "top_p"])
def test_tokens_lie_in_the_kept_set_of_each_steps_logits(model, flt):
    steps, worst = 8, 0.0
    with torch.no_grad():
        s = _session(model, steps, use_graph=False, **flt, **SAMPLE)
        for i in range(steps):
            s.step(1)
            logits = s.logits.cpu()
            y = R.pick_value(logits, T)
            rows = [R.classes(y[r]) for r in range(3)]
            worst = max(worst, _check(y, rows, s.pred_ids[i].cpu(), s.pred_cut_y[i].cpu(), s.pred_n_kept[i].cpu(), flt))
    print(f"session {flt}: largest deviation {worst:.3g}")
    assert worst <= EPS


def test_top_k_1_is_greedy_up_to_ties(model):
    steps = 8
    with torch.no_grad():
        greedy = _session(model, steps, use_graph=False)
        greedy.step(steps)
        s = _session(model, steps, use_graph=False, top_k=1, **dict(SAMPLE, temperature=1.0))
        alive = [True] * 3
        for i in range(steps):
            s.step(1)
            lg = s.logits.float().cpu()
            for r in range(3):
                t = int(s.pred_ids[i, r])
                assert float(lg[r, t]) == float(lg[r].max()), f"step {i} sample {r}: logit[id] is not the row maximum"
                if alive[r] and t != int(greedy.pred_ids[i, r]):
                    # the only way to differ from greedy: the maximum is tied and the noise chose another column of the top class
                    assert int((lg[r] == lg[r].max()).sum()) > 1, f"step {i} sample {r}: differs from greedy without a tie"
                    alive[r] = False
            assert (s.pred_n_kept[i] >= 1).all()


def test_logprobs_stay_untruncated(model):
    ops = _ops()
    steps, worst = 6, 0.0
    with torch.no_grad():
        s = _session(model, steps, use_graph=False, logprobs=True, **COMBINED, **SAMPLE)
        for i in range(steps):
            s.step(1)
            want = ops.token_logprob(s.logits, s.pred_ids[i].contiguous(), T)
            ref = LR.logprob(s.logits, s.pred_ids[i], T)
            worst = max(worst, (s.pred_logprobs[i] - want).abs().max().item(), (s.pred_logprobs[i].double().cpu() - ref).abs().max().item())
        g = _session(model, steps, use_graph=True, logprobs=True, **COMBINED, **SAMPLE)
        g.step(steps)
    assert torch.equal(g.pred_ids, s.pred_ids) and torch.equal(g.pred_logprobs, s.pred_logprobs)
    print(f"logprobs with filters: largest |error| {worst:.3g}")
    assert worst <= 1e-4


def test_refusals(model, monkeypatch):
    with pytest.raises(ValueError, match="do_sample"):
        _session(model, 4, use_graph=False, top_k=5)
    with pytest.raises(ValueError, match="top_p"):
        _session(model, 4, use_graph=False, top_p=0.0, **SAMPLE)
    with pytest.raises(ValueError, match="64 samples"):
        _session(model, 2, B=65, use_graph=False, top_k=5, **SAMPLE)
    with monkeypatch.context() as mp:
        mp.setenv("UMV_DECODE_FUSED_ARGMAX", "0")
        with pytest.raises(ValueError, match="UMV_DECODE_FUSED_ARGMAX"):
            _session(model, 4, use_graph=False, min_p=0.1, **SAMPLE)


def test_batcher_top_k_1_returns_the_greedy_answers(model):
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.serving import ContinuousBatcher
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    g = torch.Generator().manual_seed(21)
    reqs = [([torch.randn(3, 42, 56, generator=g).clamp(-1, 1)] if i % 2 == 0 else [], f"{5 + i} {17 + 3 * i} {40 + i}") for i in range(5)]
    ident = lambda x: x   # noqa: E731

    def serve(**kw):
        srv = ContinuousBatcher(model, tok, NEW_TOKEN_IDS, ident, slots=3, max_context=256, max_new_tokens=6, check_every=4, **kw)
        rids = [srv.submit(images, prompt) for images, prompt in reqs]
        got = srv.run()
        return [got[r] for r in rids]
    assert serve(do_sample=True, top_k=1) == serve(), "top_k = 1 differs from greedy: possible only where a step's maximum is tied"


def test_vqa_inferencer_config_keys(model):
    from PIL import Image
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.interactive_vqa_inferencer import VQAInferencer
    from unimedvl_amd.transforms import ImageTransform
    v = VQAInferencer({"max_new_tokens": 6, "do_sample": True, "temperature": T, "top_p": 0.9, "top_k": 20})
    v.load_model(model=model, tokenizer=ToyTokenizer(NEW_TOKEN_IDS), new_token_ids=NEW_TOKEN_IDS)
    v.image_transform = ImageTransform(56, 28, 14)
    pil = Image.fromarray(np.random.default_rng(3).integers(0, 255, (60, 84, 3), dtype=np.uint8))
    torch.manual_seed(5)
    a = v.infer_single(pil, "5 6 7 8")
    torch.manual_seed(5)
    b = v.infer_single(pil, "5 6 7 8")
    torch.manual_seed(5)
    c = v.infer_single(pil, "5 6 7 8", top_k=1, top_p=1.0)
    assert isinstance(a["answer"], str) and a["answer"] == b["answer"] and isinstance(c["answer"], str)
    with pytest.raises(ValueError, match="min_p"):
        v.infer_single(pil, "5 6 7 8", min_p=2.0)
