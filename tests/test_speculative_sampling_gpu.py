"""Sampled speculative decode on the GPU (include/unimedvl_hip.h, "speculative decode with sampling"; unimedvl_amd/speculative.py).

1. umv_decode_pick_rows against umv_decode_step_end_rows: picks, logprob, cut_y, n_kept bit for bit on copies of the same buffers, the
   keys, statistics and logits being what the real per-row lm_head call leaves for crafted weights; the table and the logits are
   untouched; the refusals.
2. umv_decode_step_end_speculative_rows against the plain-Python model (tests/spec_sample_ref.py), every output word, the draws of all
   table rows and out_logprobs included, six steps in a row.
3. The host restatement of the noise held to the device: argmax(y + g_host) is the device pick on unfiltered sampled rows wherever the
   host's top-two noisy margin exceeds 1e-3 (fp32 against fp64 logarithms).
4. SpeculativeDecodeSession(sampling=...) at the tiny configuration: whatever the drafts, every emitted token is the pick of an eager
   plain DecodeSession(row_sampling=..., same seeds and streams) fed the same tokens, or a flip inside the margin the project's 0.25
   logit tolerance allows; at most 1 token in 50 may be a flip.
5. generate_text / chat / VQAInferencer with sampling, with and without draft_len; the refusals.
"""
import ctypes
import functools
import math
import random

import numpy as np
import pytest
import torch

import spec_sample_ref as R
import test_speculative_gpu as G
from conftest import NEW_TOKEN_IDS

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
ERR_ARG = -1
SEED = 90210
KDIM = 64
PROMPTS, TOKENS = G.PROMPTS, G.TOKENS


def _ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd import ops
    return ops


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32).tolist() if t.dtype == torch.float32 else t.view(torch.int16).tolist() if t.dtype == BF16 else t.tolist()


# ----------------------------------------------------------------------------- 1. the pick kernel
# (temperature, top_k, top_p, min_p) and how the row's logits are crafted
KINDS = [("greedy", (0.0, 0, 1.0, 0.0), "normal"), ("plain", (0.8, 0, 1.0, 0.0), "normal"), ("top_k", (0.8, 5, 1.0, 0.0), "normal"),
         ("top_p", (1.0, 0, 0.8, 0.0), "normal"), ("min_p", (0.7, 0, 1.0, 0.05), "normal"), ("all", (0.7, 20, 0.9, 0.02), "normal"),
         ("peaked", (0.9, 3, 0.9, 0.0), "peaked"), ("flat", (1.0, 1, 1.0, 0.0), "flat"), ("tied", (0.0, 0, 1.0, 0.0), "tied"),
         ("minus_inf", (0.8, 0, 0.9, 0.0), "minus_inf"), ("nan", (0.8, 4, 1.0, 0.0), "nan"), ("tied_sampled", (0.8, 2, 1.0, 0.0), "tied")]


def _table(pars, streams, draws, seed=SEED):
    from unimedvl_amd import sampling
    t = np.zeros(len(pars), dtype=sampling.ROW_DTYPE)
    for i, (temp, top_k, top_p, min_p) in enumerate(pars):
        t[i] = (seed, draws[i], streams[i], temp, top_k, top_p, min_p, 1.0, 0.0, 0.0)
    return sampling.to_tensor(t, "cuda")


def _lm_head(T, V, kinds, lse=True):
    """The real per-row lm_head call for T rows of crafted logits: x = e_r, so row r's logits are column r of the weight - exactly the
    bf16 values put there - plus a residual that carries the -inf columns and the NaN.  Returns (kinds per row, table, keys, stats,
    logits)."""
    ops = _ops()
    g = torch.Generator().manual_seed(V * 7 + T)
    w = torch.zeros((V, KDIM))
    res = torch.zeros((T, V))
    rows = [kinds[(r + 5) % len(kinds)] if T < len(kinds) else kinds[r % len(kinds)] for r in range(T)]
    for r, (_, _, craft) in enumerate(rows):
        col = torch.randn(V, generator=g) * 2
        if craft == "peaked":
            col[(37 * r + 11) % V] = 20.0
        elif craft == "flat":
            col = 1.0 + torch.randn(V, generator=g) * 0.02
        elif craft == "tied":
            col = col.clamp(max=5.0)
            col[(13 * r + 3) % V] = col[(13 * r + 3) % V + 7 if (13 * r + 3) % V + 7 < V else 1] = 6.0
        elif craft == "minus_inf":
            res[r, (5 * r) % (V - 40):(5 * r) % (V - 40) + 33] = float("-inf")
        elif craft == "nan":
            res[r, (29 * r + 1) % V] = float("nan")
        w[:, r] = col
    x = torch.zeros((T, KDIM), dtype=BF16, device="cuda")
    x[torch.arange(T), torch.arange(T)] = 1.0
    table = _table([p for _, p, _ in rows], [r % 5 for r in range(T)], [3 * r + 1 for r in range(T)])
    nt = (V + 15) // 16
    keys = torch.zeros((T, nt), dtype=torch.int64, device="cuda")
    stats = torch.full((T, nt, 2), 55.0, dtype=torch.float32, device="cuda") if lse else None
    logits = torch.empty((T, V), dtype=BF16, device="cuda")
    ops.gemm(x, ops.PackedLinear.from_weight(w.to(BF16).cuda()), out=logits, argmax_partial=keys, lse_partial=stats, sample_rows=table,
             residual=res.to(BF16).cuda())
    return rows, table, keys, stats, logits


def _step_end_rows(table, keys, stats, logits):
    """what umv_decode_step_end_rows leaves for these rows (on copies): picks, logprob, cut_y, n_kept of row 0 of its [max_len, B] logs"""
    ops = _ops()
    T, dev = keys.shape[0], "cuda"
    i32 = lambda v: torch.full((T,), v, dtype=torch.int32, device=dev)          # noqa: E731
    ids = torch.full((T,), -5, dtype=torch.int64, device=dev)
    in_ids, pred = torch.full((2, T), -7, dtype=torch.int64, device=dev), torch.full((2, T), -9, dtype=torch.int64, device=dev)
    lp = torch.full((2, T), 99.0, dtype=torch.float32, device=dev) if stats is not None else None
    cut, kept = torch.full((2, T), 77.0, dtype=torch.float32, device=dev), torch.full((2, T), -3, dtype=torch.int32, device=dev)
    ops.decode_step_end_rows(i32(10), i32(20), i32(11), keys.clone(), ids, in_ids, pred, torch.zeros(T, dtype=torch.int64, device=dev),
                             logits.clone(), table.clone(), lse_partial=None if stats is None else stats.clone(), logprobs=lp, cut_y=cut,
                             n_kept=kept)
    assert torch.equal(ids, pred[0])
    return pred[0], None if lp is None else lp[0], cut[0], kept[0]


def _pick_rows(table, keys, stats, logits):
    ops = _ops()
    T, dev = keys.shape[0], "cuda"
    picks = torch.full((T,), -5, dtype=torch.int64, device=dev)
    lp = torch.full((T,), 99.0, dtype=torch.float32, device=dev) if stats is not None else None
    cut, kept = torch.full((T,), 77.0, dtype=torch.float32, device=dev), torch.full((T,), -3, dtype=torch.int32, device=dev)
    ops.decode_pick_rows(keys, logits, table, picks, lse_partial=stats, logprob=lp, cut_y=cut, n_kept=kept)
    return picks, lp, cut, kept


@pytest.mark.parametrize("T", [1, 12, 64])
@pytest.mark.parametrize("V", [330, 4112])            # 20 full tiles and one of 10 columns; 257 tiles, more than a 256-thread stride
def test_pick_rows_is_the_step_ends_pick(V, T):
    rows, table, keys, stats, logits = _lm_head(T, V, KINDS)
    lc = logits.float().cpu()
    for r, (name, _, craft) in enumerate(rows):          # the crafted rows are what they are meant to be
        if craft == "minus_inf":
            assert int((lc[r] == float("-inf")).sum()) == 33
        if craft == "nan":
            assert int(torch.isnan(lc[r]).sum()) == 1
        if craft == "tied":
            assert int((lc[r] == lc[r].max()).sum()) == 2
    before = [t.clone() for t in (table, keys, stats, logits)]
    want = _step_end_rows(table, keys, stats, logits)
    got = _pick_rows(table, keys, stats, logits)
    for t, b, name in zip((table, keys, stats, logits), before, ("table", "keys", "statistics", "logits")):
        assert _bits(t) == _bits(b), f"the pick launch wrote to the {name}"
    for g, w, name in zip(got, want, ("picks", "logprob", "cut_y", "n_kept")):
        assert _bits(g) == _bits(w), f"{name}: {g.tolist()} vs {w.tolist()}"
    picks = got[0].tolist()
    assert all(0 <= p < V for p in picks)
    # without log-probabilities: the same picks and cutoffs
    got2 = _pick_rows(table, keys, None, logits)
    assert got2[1] is None and all(_bits(a) == _bits(b) for a, b in zip((got2[0], got2[2], got2[3]), (got[0], got[2], got[3])))
    # what the rows were crafted for: a peaked row keeps the fused pick, a flat row (top_k = 1 of ~equal logits) is re-drawn from the
    # kept set, a NaN column wins, a greedy tie goes to the lowest column, an unfiltered row reports -inf / V
    fused = [0xFFFFFFFF - (int(v) & 0xFFFFFFFF) for v in keys.cpu().numpy().view(np.uint64).max(axis=1)]
    cut, kept = got[2].tolist(), got[3].tolist()
    redrawn = 0
    for r, (name, par, craft) in enumerate(rows):
        if name in ("greedy", "plain", "tied"):
            assert picks[r] == fused[r] and cut[r] == float("-inf") and kept[r] == V
        if name == "tied":
            assert picks[r] == int(lc[r].argmax())
        if name == "peaked":
            assert picks[r] == fused[r] == (37 * r + 11) % V
        if name == "flat":
            redrawn += picks[r] != fused[r]
            assert lc[r, picks[r]] == lc[r].max() and kept[r] == int((lc[r] == lc[r].max()).sum())
        if name == "nan":
            assert picks[r] == (29 * r + 1) % V and math.isnan(cut[r]) and math.isnan(got[1][r].item())
        if name == "minus_inf":
            assert lc[r, picks[r]] > float("-inf") and math.isfinite(got[1][r].item())
        if name == "tied_sampled":
            assert kept[r] >= 2
    if T >= 12:
        assert redrawn > 0, "no flat row took the kept-set path"


def test_pick_rows_refusals():
    from unimedvl_amd import _lib
    lib = _lib.load()
    V, T = 330, 4
    rows, table, keys, stats, logits = _lm_head(T, V, KINDS)
    picks = torch.full((T,), -5, dtype=torch.int64, device="cuda")
    lp = torch.zeros((T,), dtype=torch.float32, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())         # noqa: E731

    def call(keys_=keys, stats_=stats, nt=21, logits_=logits, ldo=V, v=V, table_=table.data_ptr(), t=T, picks_=picks, lp_=lp):
        return lib.umv_decode_pick_rows(p(keys_), p(stats_), nt, p(logits_), ldo, v, table_, t, p(picks_), p(lp_), None, None, None)
    assert call(keys_=None) == ERR_ARG and call(logits_=None) == ERR_ARG and call(picks_=None) == ERR_ARG
    assert call(table_=None) == ERR_ARG and call(table_=table.data_ptr() + 8) == ERR_ARG             # NULL / misaligned table
    assert call(stats_=None) == ERR_ARG and call(lp_=None) == ERR_ARG                                # one without the other
    assert call(nt=20) == ERR_ARG and call(v=337) == ERR_ARG and call(ldo=V - 1) == ERR_ARG and call(nt=0) == ERR_ARG
    assert call(t=65) == ERR_ARG and call(t=-1) == ERR_ARG
    torch.cuda.synchronize()
    assert picks.tolist() == [-5] * T, "a refused call launches nothing"
    assert call(t=0) == 0 and call(stats_=None, lp_=None) == 0
    with pytest.raises(_lib.UmvError):
        _ops().decode_pick_rows(keys, logits, table, picks, lse_partial=stats)                       # statistics without logprob
    with pytest.raises(_lib.UmvError):
        _ops().decode_pick_rows(keys, logits, table[:2], picks)                                      # a table shorter than the rows


# ----------------------------------------------------------------------------- 2. the commit kernel
def _upgrade(samples):
    """spec_ref samples (as test_speculative_gpu builds them) as spec_sample_ref ones, their draws starting somewhere"""
    for b, s in enumerate(samples):
        s.__class__ = R.Sample
        s.draws = [5 * b + j for j in range(s.k + 1)]
        s.out_lp = [0.0] * len(s.out)
    return samples


class _Device(G._Device):
    def __init__(self, samples, V):
        super().__init__(samples, V)
        T = self.B * (self.k + 1)
        self.table = _table([KINDS[r % len(KINDS)][1] for r in range(T)], [r % 3 for r in range(T)], [d for s in samples for d in s.draws])
        self.out_lp = torch.zeros(self.out_ids.shape, dtype=torch.float32, device="cuda")

    def end(self, picks, row_lp, ngram, draft_only=False):
        self.picks = torch.tensor(picks, dtype=torch.int64, device="cuda")
        self.row_lp = torch.tensor(row_lp, dtype=torch.float32, device="cuda")
        _ops().decode_step_end_speculative_rows(self.tok_slot, self.tok_pos, self.kv_len, self.picks, self.table, self.ids, self.out_ids,
                                                self.n_out, self.limit, self.n_draft, self.hist, self.hist_len, self.stats, self.k, self.V,
                                                ngram=ngram, predicted=self.predicted, pred_len=self.pred_len, draft_only=draft_only,
                                                row_logprob=self.row_lp, out_logprobs=self.out_lp)

    def check(self, samples, what, table0):
        super().check(samples, what)
        k = self.k
        want = table0.clone().cpu()
        want[:, 1] = torch.tensor([d for s in samples for d in s.draws], dtype=torch.int64)
        assert torch.equal(self.table.cpu(), want), f"{what}: the table - draws {self.table[:, 1].tolist()} vs {want[:, 1].tolist()}"
        got = self.out_lp.cpu()
        for b, s in enumerate(samples):
            assert got[b].tolist() == s.out_lp, f"{what}: sample {b} out_logprobs"


@pytest.mark.parametrize("B,k", [(1, 1), (3, 3), (8, 7), (16, 3)])
def test_commit_kernel_matches_the_model(B, k):
    V = 330
    rng = random.Random(B * 100 + k * 10 + V)
    alphabet = [1, 2, 3, 4, 5, 6, 17, V - 1]
    samples = _upgrade(G._samples(B, k, V, rng))
    dev = _Device(samples, V)
    table0 = dev.table.clone()
    T = B * (k + 1)
    dev.end([0] * T, [0.0] * T, (2, 3), draft_only=True)
    for s in samples:
        s.draft()
    dev.check(samples, "first drafts", table0)                 # draft_only: the table and out_logprobs untouched
    seen = set()
    for step in range(6):
        if step == 2:              # a draft id >= V, put into the rows directly: never accepted
            tgt = min(1, B - 1)
            row = tgt * (k + 1) + 1
            samples[tgt].ids[1] = V + 3
            samples[tgt].n_draft = max(samples[tgt].n_draft, 1)
            dev.ids[row:row + 1].fill_(V + 3)
            dev.n_draft[tgt:tgt + 1].fill_(samples[tgt].n_draft)
        picks = []
        for b, s in enumerate(samples):
            policy = (b + step) % 5
            nd = s.n_draft
            mine = [rng.choice(alphabet) for _ in range(k + 1)]
            if policy == 0:            # all accepted
                mine[:nd] = s.ids[1:nd + 1]
            elif policy == 1:          # the first draft rejected
                mine[0] = next(a for a in alphabet if a != s.ids[1])
            elif policy == 2:          # rejected in the middle
                half = nd // 2
                mine[:half] = s.ids[1:half + 1]
                mine[half] = next(a for a in alphabet if a != s.ids[half + 1])
            for j in range(k + 1):
                if not 0 <= mine[j] < V:
                    mine[j] = 7
            picks += mine
        row_lp = [float(np.float32(-rng.random() * 9)) for _ in range(T)]
        dev.end(picks, row_lp, (2, 3))
        for b, s in enumerate(samples):
            before, d0 = s.n_out, s.draws[0]
            r0 = b * (k + 1)
            n, m = s.step_end(picks[r0:r0 + k + 1], row_lp[r0:r0 + k + 1])
            seen.add("m=0" if m == 0 else "clipped" if m < n + 1 else "full")
            seen.add("none" if n == 0 else "some")
            assert s.n_out == before + m and s.draws[0] == d0 + m
        dev.check(samples, f"step {step}", table0)
    if B > 1:
        assert {"m=0", "clipped", "full", "none", "some"} <= seen, seen


def test_commit_kernel_refusals():
    from unimedvl_amd import _lib
    lib = _lib.load()
    V, B, k = 330, 2, 3
    d = _Device(_upgrade(G._samples(B, k, V, random.Random(1))), V)
    T = B * (k + 1)
    picks, row_lp = torch.zeros(T, dtype=torch.int64, device="cuda"), torch.zeros(T, dtype=torch.float32, device="cuda")

    def call(step=None, **kw):
        a = _lib.SpecRowsStepArgs(step=_lib.SpecStepArgs(
            tok_slot=d.tok_slot.data_ptr(), tok_pos=d.tok_pos.data_ptr(), kv_len=d.kv_len.data_ptr(), argmax_partial=None, n_tiles=21, V=V,
            ids=d.ids.data_ptr(), out_ids=d.out_ids.data_ptr(), out_ld=d.out_ids.shape[1], n_out=d.n_out.data_ptr(), limit=d.limit.data_ptr(),
            n_draft=d.n_draft.data_ptr(), hist=d.hist.data_ptr(), hist_ld=d.hist.shape[1], hist_len=d.hist_len.data_ptr(), predicted=None,
            pred_ld=0, pred_len=None, stats=d.stats.data_ptr(), B=B, k=k, ngram_min=2, ngram_max=4, draft_only=0),
            picks=picks.data_ptr(), rows=d.table.data_ptr(), row_logprob=row_lp.data_ptr(), out_logprobs=d.out_lp.data_ptr())
        for n, v in (step or {}).items():
            setattr(a.step, n, v)
        for n, v in kw.items():
            setattr(a, n, v)
        return lib.umv_decode_step_end_speculative_rows(ctypes.byref(a), None)
    before = {n: getattr(d, n).clone() for n in ("ids", "tok_slot", "kv_len", "n_out", "stats", "hist_len", "table")}
    assert call(step=dict(k=0)) == ERR_ARG and call(step=dict(B=17)) == ERR_ARG and call(step=dict(B=1, k=64)) == ERR_ARG
    assert call(step=dict(ngram_min=0)) == ERR_ARG and call(step=dict(n_tiles=20)) == ERR_ARG
    for ptr in ("tok_slot", "tok_pos", "kv_len", "ids", "out_ids", "n_out", "limit", "n_draft", "hist", "hist_len", "stats"):
        assert call(step={ptr: None}) == ERR_ARG, ptr
    assert call(picks=None) == ERR_ARG and call(rows=None) == ERR_ARG and call(rows=d.table.data_ptr() + 8) == ERR_ARG
    assert call(row_logprob=None) == ERR_ARG and call(out_logprobs=None) == ERR_ARG              # one without the other
    torch.cuda.synchronize()
    for n, v in before.items():
        assert torch.equal(getattr(d, n), v), n         # a refused call launches nothing
    assert call(step=dict(B=0)) == 0
    assert call(step=dict(draft_only=1), picks=None, row_logprob=None, out_logprobs=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(d.table, before["table"])


# ----------------------------------------------------------------------------- 3. the host noise model held to the device
def test_host_noise_model_is_the_devices():
    left_out = rows_seen = 0
    for V in (330, 4112):
        kinds, table, keys, stats, logits = _lm_head(64, V, [("plain", (0.8, 0, 1.0, 0.0), "normal"), ("warm", (1.3, 0, 1.0, 0.0), "normal")])
        picks = _pick_rows(table, keys, stats, logits)[0].tolist()
        from unimedvl_amd import sampling
        tab = sampling.from_tensor(table)
        lc = logits.float().cpu()
        for r in range(64):
            temp = torch.tensor(float(tab["temperature"][r]), dtype=torch.float32)
            y = (lc[r] / temp).to(BF16).double().numpy()
            noisy = y + np.array(R.gumbels(int(tab["seed"][r]), int(tab["draw"][r]), int(tab["stream"][r]), V))
            order = np.argsort(-noisy)
            rows_seen += 1
            if noisy[order[0]] - noisy[order[1]] > 1e-3:
                assert picks[r] == int(order[0]), f"V={V} row {r}: device {picks[r]}, host {int(order[0])}"
            else:
                left_out += 1
    print(f"host noise model: {left_out} of {rows_seen} rows inside the 1e-3 margin (left out)")
    assert left_out * 50 <= rows_seen


# ----------------------------------------------------------------------------- the engine, at the tiny configuration
@pytest.fixture(scope="module")
def model(tiny_weights):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.config import UniMedVLConfig
    cfg, sd, _, _ = tiny_weights
    return Bagel(UniMedVLConfig.from_dict(cfg), lambda n: sd[n], device="cuda", visual_gen=False)


def _params(name):
    from unimedvl_amd.sampling import SamplingParams as P
    return {"T0.8": [P(do_sample=True, temperature=0.8)] * 3,
            "top_p": [P(do_sample=True, temperature=1.0, top_p=0.9)] * 3,
            "top_k_min_p": [P(do_sample=True, temperature=0.7, top_k=20, min_p=0.05)] * 3,
            "mixed": [P(do_sample=True, temperature=0.8), P(), P(do_sample=True, temperature=0.7, top_k=20, min_p=0.05)],
            "greedy": [P()] * 3}[name]


@functools.lru_cache(maxsize=None)
def _plain_rows(model, name, prompts_key="PROMPTS", nsplit=None):
    """the plain per-row session's 24 tokens per sample ([B][24]) and their log-probabilities ([B][24])"""
    prompts = PROMPTS if prompts_key == "PROMPTS" else G.PROMPTS5
    sess = G._plain(model, prompts=prompts, row_sampling=_params(name), seed=SEED, logprobs=True, nsplit=nsplit)
    with torch.no_grad():
        sess.step(TOKENS)
    return sess.pred_ids.t().tolist(), sess.pred_logprobs.t().cpu()


def _flips(model, prompts, tokens, params, what, strict=True):
    """tokens [rows][B]: feed them to an eager plain per-row session (same seeds and streams) and hold each to that step's pick: equal,
    or a flip inside the margin two logits each off by 0.25 allow.  Returns (flips, outside the margin, count)."""
    from unimedvl_amd import sampling
    rows = len(tokens)
    forced = torch.tensor(tokens, dtype=torch.int64)
    sess = G._plain(model, rows, prompts, use_graph=False, forced_ids=forced, row_sampling=params, seed=SEED)
    tab = sampling.from_tensor(sess.row_table)
    flips = outside = 0
    with torch.no_grad():
        for s in range(rows):
            sess.step(1)
            lg = sess.logits.float().cpu()
            pred, cut = sess.pred_ids[s].tolist(), sess.pred_cut_y[s].tolist()
            for b in range(lg.shape[0]):
                p, t = int(pred[b]), int(forced[s, b])
                if p == t:
                    continue
                flips += 1
                par = params[b]
                if not par.do_sample:
                    ok, margin = float(lg[b, p] - lg[b, t]) <= 0.25, float(lg[b, p] - lg[b, t])
                else:
                    temp = torch.tensor(par.temperature, dtype=torch.float32)
                    y = (lg[b] / temp).to(BF16).double()
                    key = R.row_key(int(tab["seed"][b]), s, int(tab["stream"][b]))
                    margin = (float(y[p]) + R.gumbel(key, p)) - (float(y[t]) + R.gumbel(key, t))
                    ok = margin <= 0.5 / par.temperature
                    if par.truncated:
                        ok = ok and float(y[t]) >= cut[b] - 0.25 / par.temperature
                if not ok:
                    outside += 1
                    assert not strict, f"{what}: step {s} sample {b}: token {t}, plain pick {p}, noisy margin {margin:.3f}"
    return flips, outside, rows * forced.shape[1]


def _drafts(model, name, drafts, k):
    if drafts == "random":
        return dict(predicted_ids=torch.randint(5, 290, (3, TOKENS), generator=torch.Generator().manual_seed(17 + k)))
    if drafts == "perfect":
        return dict(predicted_ids=_plain_rows(model, name)[0])
    return {}


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("drafts", ["random", "perfect", "empty"])
@pytest.mark.parametrize("name", ["T0.8", "top_p", "top_k_min_p", "mixed"])
def test_session_emits_the_plain_sessions_tokens(model, name, drafts, k):
    from unimedvl_amd import sampling
    params = _params(name)
    plain, plain_lp = _plain_rows(model, name)
    sess = G._spec(model, k, use_graph=True, sampling=params, seed=SEED, logprobs=True, **_drafts(model, name, drafts, k))
    assert sess.graph is not None and sess.row_table.shape == (3 * (k + 1), 6) and sess.lse_part.shape[0] == 3 * (k + 1)
    assert sess.row_cut_y.shape == sess.row_n_kept.shape == (3 * (k + 1),) and sess.out_logprobs.shape == (3, TOKENS)
    trace = G._run(sess)
    out, stats = sess.out_ids.t().tolist(), sess.stats.cpu()
    flips, _, count = _flips(model, PROMPTS, out, params, f"{name} {drafts} drafts k={k}")
    same = sess.out_ids.tolist() == plain
    print(f"sampled speculation {name} {drafts} k={k}: {flips} of {count} tokens are flips; equal to the plain run: {same}; "
          f"{len(trace)} steps, stats {stats.tolist()}")
    assert flips * 50 <= count
    # the table: sample b's rows repeat its parameters, seed and stream, and end at draw = n_out[b] + j
    tab, n_out = sampling.from_tensor(sess.row_table), sess.n_out.tolist()
    want = sampling.pack([p for p in params for _ in range(k + 1)], seed=SEED, streams=[b for b in range(3) for _ in range(k + 1)],
                         draws=[n_out[b] + j for b in range(3) for j in range(k + 1)])
    assert tab.tobytes() == want.tobytes()
    if flips == 0:
        assert same, "no flip, yet the output differs from the plain session's"
        err = (sess.out_logprobs.cpu() - plain_lp).abs().max().item()
        print(f"  log-probabilities against the plain session: largest |difference| {err:.3g}")
        assert err <= 1e-4
        if drafts == "perfect":
            assert len(trace) == R.S.steps_for(TOKENS, k) and torch.equal(stats[:, 1], stats[:, 2]) and int(stats[0, 1]) > 0
    if drafts == "empty":
        assert sess.predicted is None


@pytest.mark.parametrize("k", [1, 3, 7])
def test_graph_replay_equals_eager(model, k):
    params = _params("mixed")
    runs = []
    for graph in (True, False):
        sess = G._spec(model, k, use_graph=graph, sampling=params, seed=SEED, logprobs=True, **_drafts(model, "mixed", "random", k))
        runs.append((G._run(sess), sess.out_ids.tolist(), sess.stats.tolist(), _bits(sess.out_logprobs), sess.row_table.tolist()))
    assert runs[0] == runs[1], "graph replay differs from eager"


@pytest.mark.parametrize("k", [1, 3, 7])
def test_greedy_entries_are_the_greedy_speculative_session(model, k):
    """sampling=[SamplingParams()] * B: the greedy session's out_ids, stats and K / V^T bit for bit - and its log-probabilities on top"""
    kw = dict(draft_ngram=(1, 4), draft_context_ids=PROMPTS)
    a = G._spec(model, k, use_graph=True, **kw)
    b = G._spec(model, k, use_graph=True, sampling=_params("greedy"), logprobs=True, **kw)
    G._run(a)
    G._run(b)
    assert a.out_ids.tolist() == b.out_ids.tolist() and a.stats.tolist() == b.stats.tolist() and a.n_draft.tolist() == b.n_draft.tolist()
    a.commit(TOKENS)
    b.commit(TOKENS)
    for l in range(model.cfg.layers):
        assert torch.equal(a.cache.packed_keys(l), b.cache.packed_keys(l)) and torch.equal(a.cache.packed_values(l), b.cache.packed_values(l)), \
            f"layer {l}"
    lp = b.out_logprobs.cpu()
    assert torch.isfinite(lp).all() and (lp <= 0).all() and (lp < 0).any()


def test_control_flips_between_two_key_splits(model):
    """The reference's own noise: the plain per-row session at two key splits, one held to the other under the same clause (printed,
    not asserted: it says how many flips the sampled speculative session's different key split alone can explain)."""
    for name in ("T0.8", "top_p", "top_k_min_p", "mixed"):
        a = _plain_rows(model, name, nsplit=1)[0]
        flips, outside, count = _flips(model, PROMPTS, torch.tensor(a).t().tolist(), _params(name), f"control {name}", strict=False)
        print(f"control {name}: nsplit = 1 held to the default split: {flips} of {count} tokens are flips, {outside} outside the margin")


# ----------------------------------------------------------------------------- 5. generate_text / chat / VQAInferencer
def _gen(model, **kw):
    cache, gi = G._ctx(model, G.PROMPTS5)
    with torch.no_grad():
        return model.generate_text(past_key_values=cache, max_length=TOKENS, **gi, **kw), cache


def _params5(name):
    from unimedvl_amd.sampling import SamplingParams as P
    return [P(do_sample=p.do_sample, temperature=p.temperature, top_k=p.top_k, top_p=p.top_p, min_p=p.min_p, seed=SEED + b)
            for b, p in enumerate(_params(name))]


def test_generate_text_with_sampling_is_the_rows_session(model):
    params = _params5("mixed")
    (ids, lp), _ = _gen(model, sampling=params, return_logprobs=True)
    sess = G._plain(model, prompts=G.PROMPTS5, row_sampling=params, logprobs=True)
    with torch.no_grad():
        sess.step(TOKENS)
    assert torch.equal(ids, sess.in_ids) and _bits(lp) == _bits(sess.pred_logprobs)
    one, _ = _gen(model, sampling=params[0])                 # one SamplingParams serves every sample
    assert torch.equal(one[:, 0], ids[:, 0]) and one.shape == ids.shape
    # a seed of None is derived from the device generator: reproducible after manual_seed, new on the next call
    from unimedvl_amd.sampling import SamplingParams as P
    free = P(do_sample=True, temperature=1.5)
    torch.manual_seed(5)
    a, _ = _gen(model, sampling=free)
    b, _ = _gen(model, sampling=free)
    torch.manual_seed(5)
    c, _ = _gen(model, sampling=free)
    assert torch.equal(a, c) and not torch.equal(a, b)


@pytest.mark.parametrize("eos", [None, "sample0", "per_sample"])
@pytest.mark.parametrize("k", [1, 3])
def test_generate_text_with_sampling_and_drafts(model, k, eos):
    params = _params5("mixed")
    base, _ = _gen(model, sampling=params)
    kw = {}
    if eos is not None:       # stop on a token the plain run emits early (sample 0) / somewhere for every sample
        kw = dict(end_token_id=int(base[3, 0]), per_sample_eos=eos == "per_sample")
    (plain, plain_lp), cache0 = _gen(model, sampling=params, return_logprobs=True, **kw)
    (got, lp), cache1 = _gen(model, sampling=params, return_logprobs=True, draft_len=k, draft_ngram=(1, 4), draft_context_ids=G.PROMPTS5, **kw)
    stats = model.last_draft_stats
    flips, _, count = _flips(model, G.PROMPTS5, got[1:].tolist(), params, f"generate_text k={k} eos={eos}") if got.shape[0] > 1 else (0, 0, 0)
    print(f"generate_text sampling k={k} eos={eos}: rows {got.shape[0]} (plain {plain.shape[0]}), stats {stats.tolist()}, "
          f"{flips} of {count} tokens are flips")
    assert got.dtype == plain.dtype and got.device == plain.device and torch.equal(got[0], plain[0]) and flips * 50 <= count
    assert got.shape == plain.shape and cache1.lens == cache0.lens
    assert lp.shape == plain_lp.shape and lp.dtype == plain_lp.dtype
    if flips == 0:
        assert torch.equal(got, plain)
        assert (lp - plain_lp).abs().max().item() <= 1e-4
    if eos is None:
        assert got.shape[0] == TOKENS and int(stats[:, 0].max()) <= TOKENS


def test_chat_and_the_inferencer_with_sampling(model):
    import numpy as np
    from PIL import Image
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.interactive_vqa_inferencer import VQAInferencer
    from unimedvl_amd.sampling import SamplingParams as P
    from unimedvl_amd.transforms import ImageTransform
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    ident = lambda x: x   # noqa: E731
    img = torch.randn(3, 28, 42, generator=torch.Generator().manual_seed(2)).clamp(-1, 1)
    prompt = " ".join(str(t) for t in G.REPEATING)
    sp = P(do_sample=True, temperature=0.8, top_p=0.95, seed=77)
    plain = model.chat(tok, NEW_TOKEN_IDS, ident, [img], prompt, max_length=TOKENS, sampling=sp)
    assert plain == model.chat(tok, NEW_TOKEN_IDS, ident, [img], prompt, max_length=TOKENS, sampling=sp), "a seeded request repeats"
    for k in (1, 3):
        ans, ids, lps = model.chat(tok, NEW_TOKEN_IDS, ident, [img], prompt, max_length=TOKENS, sampling=sp, draft_len=k,
                                   draft_ngram=(1, 4), return_logprobs=True)
        print(f"chat sampling k={k}: stats {model.last_draft_stats.tolist()}")
        assert ans == plain and len(ids) == len(lps)
    pil = Image.fromarray(np.random.default_rng(3).integers(0, 255, (60, 84, 3), dtype=np.uint8))

    def make(**cfg):
        v = VQAInferencer(dict({"max_new_tokens": 10}, **cfg))          # (the default config samples: "do_sample": True)
        v.load_model(model=model, tokenizer=tok, new_token_ids=NEW_TOKEN_IDS)
        v.image_transform = ImageTransform(56, 28, 14)
        return v
    a = make(sampling=sp).infer_single(pil, "5 6 7 8")["answer"]
    assert a == make(sampling=dict(do_sample=True, temperature=0.8, top_p=0.95, seed=77)).infer_single(pil, "5 6 7 8")["answer"]
    assert a == make(sampling=sp, draft_len=2, draft_ngram=(1, 4)).infer_single(pil, "5 6 7 8")["answer"]
    with pytest.raises(ValueError, match="sampling excludes"):
        make(sampling=sp).infer_single(pil, "5 6 7 8", temperature=0.5)


def test_new_refusals(model, monkeypatch):
    from unimedvl_amd.sampling import SamplingParams as P
    sp = P(do_sample=True, temperature=0.8)

    def gen(**kw):
        cache, gi = G._ctx(model)
        with torch.no_grad():
            return model.generate_text(past_key_values=cache, max_length=4, **gi, **kw)
    for kw in (dict(do_sample=True), dict(temperature=0.7), dict(top_k=5), dict(top_p=0.9), dict(min_p=0.1), dict(repetition_penalty=1.2),
               dict(presence_penalty=0.5), dict(frequency_penalty=0.5)):
        for k in (0, 2):
            with pytest.raises(ValueError, match="sampling excludes"):
                gen(sampling=sp, draft_len=k, **kw)
    with pytest.raises(ValueError, match="one per sample"):
        gen(sampling=[sp, sp])
    for kw in (dict(return_logits=True), dict(top_logprobs=2), dict(logit_bias={7: -1.0}), dict(sampling=P(presence_penalty=0.5))):
        with pytest.raises(ValueError):
            gen(**dict(dict(sampling=sp, draft_len=2), **kw))
    with pytest.raises(ValueError, match="greedy only"):
        gen(draft_len=2, do_sample=True)
    for kw in (dict(sampling=P(repetition_penalty=1.1)), dict(sampling=sp, logit_bias={3: 1.0}),
               dict(sampling=sp, forced_ids=torch.zeros((4, 3), dtype=torch.int64)), dict(sampling=sp, top_logprobs=2),
               dict(sampling=[sp] * 2), dict(sampling_streams=[0, 1, 2])):
        with pytest.raises(ValueError):
            G._spec(model, 2, steps=4, use_graph=False, **kw)
    with pytest.raises(ValueError, match="64"):
        G._spec(model, 31, steps=4, use_graph=False, sampling=sp)              # 3 x 32 rows
    with monkeypatch.context() as mp:
        mp.setenv("UMV_DECODE_FUSED_ARGMAX", "0")
        with pytest.raises(ValueError, match="UMV_DECODE_FUSED_ARGMAX"):
            G._spec(model, 2, steps=4, use_graph=False, sampling=sp)
    assert gen(sampling=sp, draft_len=2, return_logprobs=True)[1].shape == (4, 3)
