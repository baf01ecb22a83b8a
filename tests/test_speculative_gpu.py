"""Speculative greedy decode on the GPU (include/unimedvl_hip.h, "speculative greedy decode"; unimedvl_amd/speculative.py).

1. umv_decode_step_end_speculative against the plain-Python model (tests/spec_ref.py), bit for bit on every output word, over several
   steps in a row, with keys the real lm_head call leaves for crafted logits.
2. umv_attn_varlen at the step's shape (max_q = k + 1, key split, causal) against fp64 attention, to the absolute bound
   tests/test_kernels_gpu.py holds this kernel to (0.03 on N(0, 1) inputs).
3. SpeculativeDecodeSession at the tiny configuration: perfect predictions are all accepted in ceil(24 / (k + 1)) steps, a corrupted
   prediction gives the acceptance pattern spec_ref derives, graph replay equals eager, K / V^T stay within the engine tests' bound
   (2e-2 of the tensor's range) of the plain session's.
4. Draft invariance: whatever the drafts, every emitted token is the argmax of a plain session fed the same tokens, or lies within
   0.25 of its top logit (SURVEY.md section 8c's logit tolerance: the key split depends on the segment's length, so the last bit of a
   logit may differ); at most 1 token in 50 may need that clause.
5. generate_text / chat with draft_len: the plain call's matrix shape, stop row and cache lengths; the refusals.
"""
import ctypes
import functools
import math
import random

import pytest
import torch

import spec_ref as S
from conftest import NEW_TOKEN_IDS

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
ERR_ARG = -1


def _ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd import ops
    return ops


# ----------------------------------------------------------------------------- 1. the kernel
KDIM = 64          # x = e_r: row r's logits are column r of the weight, so a logit is exactly the bf16 value put there


def _keys_for(picks, V, ties):
    """argmax keys [T, n_tiles] of the real lm_head call for logits whose row r has its maximum (20) at picks[r] - and, for r in ties,
    the same value at the HIGHER column ties[r] as well - over N(0, 1) noise clamped below 5"""
    ops = _ops()
    T = len(picks)
    g = torch.Generator().manual_seed(V * 131 + sum(picks))
    w = torch.zeros((V, KDIM))
    w[:, :T] = torch.randn(V, T, generator=g).clamp(max=5.0)
    for r, c in enumerate(picks):
        w[c, r] = 20.0
        if r in ties:
            assert ties[r] > c
            w[ties[r], r] = 20.0
    x = torch.zeros((T, KDIM), dtype=BF16, device="cuda")
    x[torch.arange(T), torch.arange(T)] = 1.0
    keys = torch.zeros((T, (V + 15) // 16), dtype=torch.int64, device="cuda")
    out = torch.empty((T, V), dtype=BF16, device="cuda")
    ops.gemm(x, ops.PackedLinear.from_weight(w.to(BF16).cuda()), out=out, argmax_partial=keys)
    assert out.float().cpu().argmax(-1).tolist() == list(picks)          # (CPU argmax: lowest index on ties)
    return keys


class _Device:
    """the kernel's buffers for a list of spec_ref.Sample, as the samples are BEFORE their first draft"""

    def __init__(self, samples, V):
        dev, B, k = "cuda", len(samples), samples[0].k
        self.B, self.k, self.V = B, k, V
        i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
        flat = lambda name: [v for s in samples for v in getattr(s, name)]     # noqa: E731
        self.ids = torch.tensor(flat("ids"), **i64)
        self.tok_slot = torch.tensor(flat("tok_slot"), **i32)
        self.tok_pos = torch.tensor(flat("tok_pos"), **i32)
        self.kv_len = torch.tensor([s.kv_len for s in samples], **i32)
        self.out_ids = torch.tensor([s.out for s in samples], **i64)
        self.n_out = torch.tensor([s.n_out for s in samples], **i32)
        self.limit = torch.tensor([s.limit for s in samples], **i32)
        self.n_draft = torch.tensor([s.n_draft for s in samples], **i32)
        self.hist = torch.tensor([s.hist for s in samples], **i32)
        self.hist_len = torch.tensor([s.hist_len for s in samples], **i32)
        self.stats = torch.tensor([s.stats for s in samples], **i32)
        self.predicted = self.pred_len = None
        if any(s.predicted is not None for s in samples):
            n = max(len(s.predicted) for s in samples if s.predicted is not None)
            self.predicted = torch.tensor([(s.predicted or []) + [-1] * (n - len(s.predicted or [])) for s in samples], **i64)
            self.pred_len = torch.tensor([s.pred_len if s.predicted is not None else 0 for s in samples], **i32)

    def end(self, keys, ngram, draft_only=False):
        _ops().decode_step_end_speculative(self.tok_slot, self.tok_pos, self.kv_len, keys, self.ids, self.out_ids, self.n_out, self.limit,
                                           self.n_draft, self.hist, self.hist_len, self.stats, self.k, self.V, ngram=ngram,
                                           predicted=self.predicted, pred_len=self.pred_len, draft_only=draft_only)

    def check(self, samples, what):
        k = self.k
        got = {n: getattr(self, n).cpu() for n in ("ids", "tok_slot", "tok_pos", "kv_len", "out_ids", "n_out", "n_draft", "hist",
                                                   "hist_len", "stats")}
        for b, s in enumerate(samples):
            rows = slice(b * (k + 1), (b + 1) * (k + 1))
            want = dict(ids=s.ids, tok_slot=s.tok_slot, tok_pos=s.tok_pos)
            for n, v in want.items():
                assert got[n][rows].tolist() == v, f"{what}: sample {b} {n}: {got[n][rows].tolist()} vs {v}"
            want = dict(kv_len=s.kv_len, out_ids=s.out, n_out=s.n_out, n_draft=s.n_draft, hist=s.hist, hist_len=s.hist_len, stats=s.stats)
            for n, v in want.items():
                assert got[n][b].tolist() == v, f"{what}: sample {b} {n}: {got[n][b].tolist()} vs {v}"


def _samples(B, k, V, rng):
    """B samples that between them start without drafts, with lookup drafts, with a predicted continuation shorter than the window or
    holding a token >= V, with a limit inside the first windows and with limit 0"""
    out = []
    alphabet = [1, 2, 3, 4, 5, 6, 17, V - 1]
    for b in range(B):
        kind = b % 4
        context, predicted = [], None
        if kind in (0, 3):         # a history with repeats and a separator: the lookup drafts from the first call on
            context = [rng.choice(alphabet) for _ in range(12)] + [-1] + [1, 2, 3, 4, 5, 6, 1, 2]
        if kind == 1:              # predicted continuation: two tokens (shorter than any window with k >= 3), or a token >= V in it
            predicted = [3, 4] if b % 8 == 1 else [5, 6, V + 5, 1, 2, 3, 4, 5]
        limit = (3 if b % 8 == 0 else 0 if b % 8 == 3 else 40)
        t0 = 3 if kind != 2 else V - 1          # kind 2: no context, no prediction - no drafts until it repeats itself
        out.append(S.Sample(k, t0, slot=10 + 3 * b, pos=100 + b, out_ld=24, limit=limit, hist=context + [t0], hist_ld=48, vocab=V,
                            ngram=(2, 3), predicted=predicted, pred_len=0 if predicted is None else len(predicted)))
    return out


@pytest.mark.parametrize("V", [330, 4112])         # 20 full tiles and one of 10 columns; 257 tiles
@pytest.mark.parametrize("B,k", [(1, 1), (3, 3), (8, 7), (16, 3)])
def test_kernel_matches_the_model(B, k, V):
    rng = random.Random(B * 100 + k * 10 + V)
    alphabet = [1, 2, 3, 4, 5, 6, 17, V - 1]
    samples = _samples(B, k, V, rng)
    dev = _Device(samples, V)
    dev.end(torch.zeros((B * (k + 1), (V + 15) // 16), dtype=torch.int64, device="cuda"), (2, 3), draft_only=True)
    for s in samples:
        s.draft()
    dev.check(samples, "first drafts")
    seen = set()
    for step in range(6):
        if step == 2:              # a draft id >= V, put into the rows directly: never accepted
            tgt = min(1, B - 1)
            row = tgt * (k + 1) + 1
            samples[tgt].ids[1] = V + 3
            samples[tgt].n_draft = max(samples[tgt].n_draft, 1)
            dev.ids[row:row + 1].fill_(V + 3)
            dev.n_draft[tgt:tgt + 1].fill_(samples[tgt].n_draft)
        picks, ties = [], {}
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
            elif policy == 3 and nd and 0 < s.ids[1] < V:      # tied maxima: the lowest column wins, the draft (the higher one) is rejected
                mine[0] = s.ids[1] - 1
                ties[b * (k + 1)] = s.ids[1]
            for j in range(k + 1):         # a pick is a token of the vocabulary (step 2's draft >= V cannot be one)
                if not 0 <= mine[j] < V:
                    mine[j] = 7
            picks += mine
        keys = _keys_for(picks, V, ties)
        dev.end(keys, (2, 3))
        for b, s in enumerate(samples):
            before = s.n_out
            n, m = s.step_end(picks[b * (k + 1):(b + 1) * (k + 1)])
            seen.add("m=0" if m == 0 else "clipped" if m < n + 1 else "full")
            seen.add("none" if n == 0 else "some")
            assert s.n_out == before + m
        dev.check(samples, f"step {step}")
    if B > 1:
        assert {"m=0", "clipped", "full", "none", "some"} <= seen, seen


def test_kernel_refusals():
    from unimedvl_amd import _lib
    lib = _lib.load()
    V, B, k = 330, 2, 3
    samples = _samples(B, k, V, random.Random(1))
    d = _Device(samples, V)
    keys = torch.zeros((B * (k + 1), 21), dtype=torch.int64, device="cuda")

    def call(**kw):
        a = _lib.SpecStepArgs(
            tok_slot=d.tok_slot.data_ptr(), tok_pos=d.tok_pos.data_ptr(), kv_len=d.kv_len.data_ptr(), argmax_partial=keys.data_ptr(),
            n_tiles=21, V=V, ids=d.ids.data_ptr(), out_ids=d.out_ids.data_ptr(), out_ld=d.out_ids.shape[1], n_out=d.n_out.data_ptr(),
            limit=d.limit.data_ptr(), n_draft=d.n_draft.data_ptr(), hist=d.hist.data_ptr(), hist_ld=d.hist.shape[1],
            hist_len=d.hist_len.data_ptr(), predicted=None, pred_ld=0, pred_len=None, stats=d.stats.data_ptr(), B=B, k=k,
            ngram_min=2, ngram_max=4, draft_only=0)
        for n, v in kw.items():
            setattr(a, n, v)
        return lib.umv_decode_step_end_speculative(ctypes.byref(a), None)
    before = {n: getattr(d, n).clone() for n in ("ids", "tok_slot", "kv_len", "n_out", "stats", "hist_len")}
    assert call(k=0) == ERR_ARG and call(k=-1) == ERR_ARG
    assert call(B=17) == ERR_ARG                       # 68 rows
    assert call(B=1, k=64) == ERR_ARG                  # 65 rows
    assert call(ngram_min=0) == ERR_ARG and call(ngram_min=5) == ERR_ARG
    for ptr in ("tok_slot", "tok_pos", "kv_len", "argmax_partial", "ids", "out_ids", "n_out", "limit", "n_draft", "hist", "hist_len", "stats"):
        assert call(**{ptr: None}) == ERR_ARG, ptr
    assert call(predicted=d.ids.data_ptr(), pred_ld=4) == ERR_ARG          # predicted without pred_len
    assert call(n_tiles=20) == ERR_ARG                 # 330 columns are 21 tiles
    torch.cuda.synchronize()
    for n, v in before.items():
        assert torch.equal(getattr(d, n), v), n         # a refused call launches nothing
    assert call(B=0) == 0
    with pytest.raises(_lib.UmvError):
        _ops().decode_step_end_speculative(d.tok_slot, d.tok_pos, d.kv_len, keys, d.ids, d.out_ids, d.n_out, d.limit, d.n_draft, d.hist,
                                           d.hist_len, d.stats, k, V, ngram=(3, 2))


# ----------------------------------------------------------------------------- 2. attention at the step's shape
@pytest.mark.parametrize("k", [1, 3, 7])       # 7 heads per KV group x (k + 1) tokens = 14 rows: one 16-row q-tile; 28 rows: two; 56: four
def test_attention_at_the_steps_shape(k):
    ops = _ops()
    nq, nkv, hd, nsplit = 28, 4, 128, 4
    ctx = [5, 33, 300]
    nseg, Q = len(ctx), k + 1
    k_lens = [c + Q for c in ctx]
    cap = (max(k_lens) + 31) // 32 * 32
    g = torch.Generator().manual_seed(60 + k)
    q = torch.randn((nseg * Q, nq, hd), generator=g).to(BF16)
    slab = ops.KVSlab(nseg, nkv, cap, hd, "cuda")
    kh, vh = torch.zeros_like(slab.k, device="cpu"), torch.zeros_like(slab.vt, device="cpu")
    ks = [torch.randn((n, nkv, hd), generator=g).to(BF16) for n in k_lens]
    vs = [torch.randn((n, nkv, hd), generator=g).to(BF16) for n in k_lens]
    for i, n in enumerate(k_lens):
        kh[i, :, :n] = ks[i].transpose(0, 1)
        vh[i, :, :, :n] = vs[i].permute(1, 2, 0)
    slab.k.copy_(kh)
    slab.vt.copy_(vh)
    cu = (torch.arange(nseg + 1, dtype=torch.int32) * Q).cuda()
    out = torch.zeros((nseg * Q, nq, hd), dtype=BF16, device="cuda")
    ws = ops.attn_workspace(nseg, nq, hd, Q, nsplit, "cuda")
    ops.attention(q.cuda(), out, slab, cu, torch.tensor(k_lens, dtype=torch.int32).cuda(), nq, nkv, hd, True, Q, max(k_lens), nsplit, ws)
    got = out.cpu().double()
    worst = 0.0
    for i, n in enumerate(k_lens):
        qs = q[i * Q:(i + 1) * Q].double()                               # [Q, nq, hd]
        kk = ks[i].double().repeat_interleave(nq // nkv, dim=1)          # [n, nq, hd]
        vv = vs[i].double().repeat_interleave(nq // nkv, dim=1)
        sc = torch.einsum("qhd,khd->hqk", qs, kk) / math.sqrt(hd)
        vis = torch.arange(n)[None, :] <= (n - Q + torch.arange(Q))[:, None]          # bottom-right causal: row j sees keys 0..ctx + j
        sc = sc.masked_fill(~vis[None], float("-inf"))
        ref = torch.einsum("hqk,khd->qhd", sc.softmax(-1), vv)
        worst = max(worst, (got[i * Q:(i + 1) * Q] - ref).abs().max().item())
    print(f"attention max_q={Q} nsplit={nsplit}: largest |error| {worst:.4g}")
    assert worst < 0.03


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
# a prompt with a repeated phrase and most of the vocabulary behind it: with draft_ngram = (1, 4) nearly any generated token is found
REPEATING = [11, 22, 33, 44] * 3 + list(range(5, 295))
TOKENS = 24


def _ctx(model, prompts=PROMPTS, paged=False):
    """a freshly prefilled cache of the prompts' text contexts and the start tokens"""
    from unimedvl_amd.kvcache import NaiveCache, PagedCache

    class Tok:
        def encode(self, s):
            return prompts[int(s)]
    B = len(prompts)
    cache = PagedCache(model.cfg.layers, pool_pages=64, max_context=2048) if paged else NaiveCache(model.cfg.layers)
    gi, kvl, rope = model.prepare_prompts([0] * B, [0] * B, [str(i) for i in range(B)], Tok(), NEW_TOKEN_IDS)
    with torch.no_grad():
        cache = model.forward_cache_update_text(cache, **gi)
    return cache, model.prepare_start_tokens(kvl, rope, NEW_TOKEN_IDS)


def _plain(model, steps=TOKENS, prompts=PROMPTS, paged=False, **kw):
    from unimedvl_amd.decode import DecodeSession
    cache, gi = _ctx(model, prompts, paged)
    with torch.no_grad():
        return DecodeSession(model.language_model, cache, gi["packed_start_tokens"], gi["packed_query_position_ids"], steps, **kw)


def _spec(model, k, steps=TOKENS, prompts=PROMPTS, paged=False, **kw):
    from unimedvl_amd.speculative import SpeculativeDecodeSession
    cache, gi = _ctx(model, prompts, paged)
    with torch.no_grad():
        return SpeculativeDecodeSession(model.language_model, cache, gi["packed_start_tokens"], gi["packed_query_position_ids"], steps, k,
                                        **kw)


@functools.lru_cache(maxsize=None)
def _plain_tokens(model, paged=False):
    """the plain session's 24 tokens per sample ([B][24]) and its committed K / V per layer"""
    sess = _plain(model, paged=paged)
    with torch.no_grad():
        sess.step(TOKENS)
    sess.commit(TOKENS)
    kv = [(sess.cache.packed_keys(l).float().cpu(), sess.cache.packed_values(l).float().cpu()) for l in range(model.cfg.layers)]
    return sess.pred_ids.t().tolist(), kv


def _run(sess):
    """step until every sample holds TOKENS tokens; returns n_out after every step"""
    trace = []
    with torch.no_grad():
        while int(sess.n_out.min()) < TOKENS:
            sess.step(1)
            trace.append(sess.n_out.tolist())
    return trace


def _derive(model, plain, predicted, k):
    """what spec_ref makes of these predictions when the model's pick after a true prefix is the plain session's token (the picks of
    rows behind a wrong draft are never looked at: -7)"""
    start = NEW_TOKEN_IDS["bos_token_id"]
    samples, traces = [], []
    for b in range(len(plain)):
        s = S.Sample(k, start, slot=0, pos=0, out_ld=TOKENS, limit=TOKENS, hist=[start], hist_ld=1 + TOKENS, vocab=model.cfg.vocab,
                     predicted=predicted[b], pred_len=len(predicted[b]))
        s.draft()
        samples.append(s)
    while min(s.n_out for s in samples) < TOKENS:
        for b, s in enumerate(samples):
            picks, true = [], True
            for j in range(k + 1):
                true = true and (j == 0 or (j <= s.n_draft and s.n_out + j - 1 < TOKENS and s.ids[j] == plain[b][s.n_out + j - 1]))
                picks.append(plain[b][s.n_out + j] if true and s.n_out + j < TOKENS else -7)
            s.step_end(picks)
        traces.append([s.n_out for s in samples])
    return samples, traces


# ----------------------------------------------------------------------------- 3. the session
@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
@pytest.mark.parametrize("k", [1, 3, 7])
def test_session_with_predictions(model, k, paged):
    plain, kv = _plain_tokens(model, paged)
    B = len(plain)
    # perfect predictions: everything drafted is accepted, in ceil(24 / (k + 1)) steps
    sess = _spec(model, k, paged=paged, predicted_ids=plain, use_graph=True)
    assert sess.graph is not None and sess.rows == B * (k + 1) and sess.out_ids.shape == (B, TOKENS)
    trace = _run(sess)
    stats = sess.stats.cpu()
    print(f"perfect predictions k={k}: {len(trace)} steps, stats {stats.tolist()}")
    assert sess.out_ids.tolist() == plain
    assert len(trace) == S.steps_for(TOKENS, k) and (stats[:, 0] == len(trace)).all()
    assert torch.equal(stats[:, 1], stats[:, 2]) and int(stats[0, 1]) > 0
    sess.commit(TOKENS)
    assert sess.cache.lens == [n + TOKENS for n in sess.lens0]
    worst = 0.0
    for l in range(model.cfg.layers):
        for mine, ref, what in ((sess.cache.packed_keys(l), kv[l][0], "K"), (sess.cache.packed_values(l), kv[l][1], "V")):
            err = (mine.float().cpu() - ref).abs().max().item() / (ref.max() - ref.min()).item()
            worst = max(worst, err)
            assert mine.shape == ref.shape and err <= 2e-2, f"layer {l} {what}: {err:.3g} of the range"
    print(f"K / V below the committed length: worst {worst:.3g} of the range")
    # one prediction corrupted per sample: the pattern spec_ref derives; graph replay == eager
    predicted = [list(p) for p in plain]
    for b, at in enumerate((3, 10, 17)):
        predicted[b][at] = (predicted[b][at] + 7) % 290 + 5
        assert predicted[b][at] != plain[b][at]
    want, want_trace = _derive(model, plain, predicted, k)
    runs = []
    for graph in (True, False):
        sess = _spec(model, k, paged=paged, predicted_ids=predicted, use_graph=graph)
        runs.append((_run(sess), sess.out_ids.tolist(), sess.stats.tolist(), sess.n_draft.tolist()))
    assert runs[0] == runs[1], "graph replay differs from eager"
    trace, out, stats, n_draft = runs[0]
    print(f"corrupted predictions k={k}: n_out per step {trace}, stats {stats}")
    assert out == plain
    assert trace == want_trace and stats == [s.stats for s in want] and n_draft == [s.n_draft for s in want]


# ----------------------------------------------------------------------------- 4. draft invariance
def _teacher_forced_flips(model, prompts, tokens, what):
    """tokens [rows][B]: feed them to an eager plain session and hold each to that step's logits: the argmax, or within 0.25 of it.
    Returns (flips, count)."""
    rows = len(tokens)
    forced = torch.tensor(tokens, dtype=torch.int64)
    sess = _plain(model, rows, prompts, use_graph=False, forced_ids=forced)
    flips = 0
    with torch.no_grad():
        for s in range(rows):
            sess.step(1)
            lg = sess.logits.float().cpu()
            for b in range(lg.shape[0]):
                top, t = int(lg[b].argmax()), int(forced[s, b])
                if top != t:
                    margin = float(lg[b, top] - lg[b, t])
                    assert margin <= 0.25, f"{what}: step {s} sample {b}: token {t}, plain argmax {top}, margin {margin:.3f}"
                    flips += 1
    return flips, rows * forced.shape[1]


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("drafts", ["random", "perfect", "empty"])
def test_draft_invariance(model, k, drafts):
    plain, _ = _plain_tokens(model)
    g = torch.Generator().manual_seed(17 + k)
    kw = {}
    if drafts == "random":
        kw["predicted_ids"] = torch.randint(5, 290, (len(plain), TOKENS), generator=g)
    elif drafts == "perfect":
        kw["predicted_ids"] = plain
    sess = _spec(model, k, use_graph=True, **kw)
    _run(sess)
    out = sess.out_ids.t().tolist()                        # [24][B]
    flips, count = _teacher_forced_flips(model, PROMPTS, out, f"{drafts} drafts k={k}")
    print(f"draft invariance {drafts} k={k}: {flips} of {count} tokens inside the 0.25 margin; equal to the plain run: "
          f"{sess.out_ids.tolist() == plain}; stats {sess.stats.tolist()}")
    assert flips * 50 <= count
    if drafts == "empty":
        assert sess.predicted is None


# ----------------------------------------------------------------------------- 5. generate_text / chat
PROMPTS5 = [REPEATING, REPEATING[4:] + [7, 8], [11, 22, 33, 44] * 5]


@pytest.mark.parametrize("eos", [None, "sample0", "per_sample"])
@pytest.mark.parametrize("k", [1, 3])
def test_generate_text_with_drafts(model, k, eos):
    def run(**kw):
        cache, gi = _ctx(model, PROMPTS5)
        with torch.no_grad():
            return model.generate_text(past_key_values=cache, max_length=TOKENS, **gi, **kw), cache
    base, _ = run()
    kw = {}
    if eos is not None:       # stop on a token the greedy run emits early (sample 0) / somewhere for every sample
        kw = dict(end_token_id=int(base[3, 0]), per_sample_eos=eos == "per_sample")
    plain, cache0 = run(**kw)
    got, cache1 = run(draft_len=k, draft_ngram=(1, 4), draft_context_ids=PROMPTS5, **kw)
    stats = model.last_draft_stats
    flips, count = _teacher_forced_flips(model, PROMPTS5, got[1:].tolist(), f"generate_text k={k} eos={eos}") if got.shape[0] > 1 else (0, 0)
    print(f"generate_text k={k} eos={eos}: rows {got.shape[0]} (plain {plain.shape[0]}), stats {stats.tolist()}, "
          f"{flips} of {count} tokens inside the 0.25 margin")
    assert got.dtype == plain.dtype and got.device == plain.device
    assert torch.equal(got[0], plain[0]) and flips * 50 <= count
    assert got.shape == plain.shape and cache1.lens == cache0.lens
    if flips == 0:
        assert torch.equal(got, plain)
    assert int(stats[:, 1].sum()) > 0, "the lookup never drafted"
    if eos is None:
        assert got.shape[0] == TOKENS and int(stats[:, 0].max()) <= TOKENS


def test_chat_with_drafts(model):
    from oracle.toy_tokenizer import ToyTokenizer
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    ident = lambda x: x   # noqa: E731
    img = torch.randn(3, 28, 42, generator=torch.Generator().manual_seed(2)).clamp(-1, 1)
    prompt = " ".join(str(t) for t in REPEATING)
    plain = model.chat(tok, NEW_TOKEN_IDS, ident, [img], prompt, max_length=TOKENS)
    for k in (1, 3):
        assert model.chat(tok, NEW_TOKEN_IDS, ident, [img], prompt, max_length=TOKENS, draft_len=k, draft_ngram=(1, 4)) == plain
        stats = model.last_draft_stats
        print(f"chat k={k}: stats {stats.tolist()}")
        assert int(stats[0, 1]) > 0, "the lookup never drafted"
        # a predicted answer, as a string: accepted as far as it is right
        assert model.chat(tok, NEW_TOKEN_IDS, ident, [img], prompt, max_length=TOKENS, draft_len=k, predicted_ids=plain) == plain
        assert int(model.last_draft_stats[0, 2]) > 0 or not plain.strip()


def test_draft_len_zero_is_the_plain_call(model, monkeypatch):
    from unimedvl_amd import bagel, speculative
    built = []

    class Plain(bagel.DecodeSession):
        def __init__(self, *a, **kw):
            built.append("plain")
            super().__init__(*a, **kw)

    class Spec(speculative.SpeculativeDecodeSession):
        def __init__(self, *a, **kw):
            built.append("speculative")
            super().__init__(*a, **kw)
    monkeypatch.setattr(bagel, "DecodeSession", Plain)
    monkeypatch.setattr(speculative, "SpeculativeDecodeSession", Spec)
    cache, gi = _ctx(model)
    with torch.no_grad():
        a = model.generate_text(past_key_values=cache, max_length=4, draft_len=0, **gi)
    assert built == ["plain"] and a.shape == (4, 3)
    cache, gi = _ctx(model)
    with torch.no_grad():
        b = model.generate_text(past_key_values=cache, max_length=4, draft_len=2, **gi)
    assert built == ["plain", "speculative"] and torch.equal(a, b)


def test_refusals(model, monkeypatch):
    def gen(**kw):
        cache, gi = _ctx(model)
        with torch.no_grad():
            return model.generate_text(past_key_values=cache, max_length=4, draft_len=2, **gi, **kw)
    for kw in (dict(do_sample=True), dict(return_logits=True), dict(return_logprobs=True), dict(repetition_penalty=1.2),
               dict(presence_penalty=0.5), dict(frequency_penalty=0.5), dict(logit_bias={7: -1.0}), dict(top_k=5, do_sample=True)):
        with pytest.raises(ValueError, match="greedy only"):
            gen(**kw)
    from unimedvl_amd.sampling import SamplingParams
    for kw in (dict(do_sample=True), dict(logprobs=True), dict(forced_ids=torch.zeros((4, 3), dtype=torch.int64)),
               dict(repetition_penalty=1.1), dict(logit_bias={3: 1.0}), dict(row_sampling=[SamplingParams()] * 3)):
        with pytest.raises(ValueError, match="greedy only"):
            _spec(model, 2, steps=4, use_graph=False, **kw)
    with pytest.raises(ValueError, match="greedy only.*64"):
        _spec(model, 31, steps=4, use_graph=False)              # 3 x 32 rows
    with pytest.raises(ValueError, match="draft_len"):
        _spec(model, 0, steps=4, use_graph=False)
    with pytest.raises(ValueError, match="draft_ngram"):
        _spec(model, 2, steps=4, use_graph=False, draft_ngram=(3, 2))
    with monkeypatch.context() as mp:
        mp.setenv("UMV_DECODE_FUSED_ARGMAX", "0")
        with pytest.raises(ValueError, match="greedy only.*UMV_DECODE_FUSED_ARGMAX"):
            _spec(model, 2, steps=4, use_graph=False)
    sess = _spec(model, 2, steps=4, use_graph=False)
    with pytest.raises(ValueError, match="set_slot"):
        sess.set_slot(0, 5, 3, 3)
