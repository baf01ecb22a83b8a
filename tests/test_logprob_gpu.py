"""Token log-probabilities from the decode step (include/unimedvl_hip.h, "token log-probabilities") on the GPU.

Bound: inputs are bf16, so y[id] and the maximum are exact; the fp32 exponentials (argument error |x| 2^-24, weighted by the softmax
mass: about ln V 2^-24), the tree sum (about 17 x 2^-24 over 152 k terms), one log and two subtractions (|logprob| 2^-23) come to
about 2e-5 for |logprob| <= 200.  Every value is asserted within BOUND = 1e-4 absolute - five times that - of the fp64 reference
(tests/logprob_ref.py) on the very logits the call stored; the per-tile sums within 1e-5 relative, the per-tile maxima exactly.

Largest errors seen on an MI355X (every test prints its own before it asserts; `pytest -s`): finished log-probability 5.6e-7 (fused,
stand-alone, session, forced session and generate_text alike; |logprob| up to ~15), s_t 2.6e-7 relative - forty times below the derived
2e-5, as expected of vocabularies of 320 .. 4112 columns where the derivation is priced for 152 k.
"""
import functools
import math

import numpy as np
import pytest
import torch

import logprob_ref as R
from conftest import NEW_TOKEN_IDS

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
BOUND = 1e-4
MS = [1, 8, 9, 16, 17, 32, 33, 64]          # one value on each side of every row class of the weight-streaming kernel
K = 512
T_SAMPLE, SEED = 0.7, 1234


def _ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _lin(kind, N, special=None):
    """kind: bf16 | fp8 | z13.  Logits of N(0, ~2.3^2): x ~ N(0, 1), w ~ N(0, 0.1^2), K = 512.  special = "-inf": a bias of -inf on
    columns 32..47 (a whole tile) and 100..103 (part of one)"""
    ops = _ops()
    g = torch.Generator().manual_seed(N + len(kind))
    w = (torch.randn(N, K, generator=g) * 0.1).to(BF16).cuda()
    b = (torch.randn(N, generator=g) * 0.5).to(BF16)
    if special == "-inf":
        b[32:48] = float("-inf")
        b[100:104] = float("-inf")
    b = b.cuda()
    if kind == "fp8":
        return ops.PackedLinear.from_weight_fp8(w, b)
    lin = ops.PackedLinear.from_weight(w, b)
    return lin.build_z13() if kind == "z13" else lin


@functools.lru_cache(maxsize=None)
def _x(rows=64):
    return torch.randn(rows, K, generator=torch.Generator().manual_seed(5)).to(BF16).cuda()


def _gemm(kind, N, M, temp, lse=True, special=None, x=None, residual=None):
    """the lm_head-form GEMM on rows [0, M) -> (logits, keys, lse or None)"""
    ops = _ops()
    lin = _lin(kind, N, special)
    x = _x()[:M] if x is None else x
    nt = (N + 15) // 16
    keys = torch.zeros((M, nt), dtype=torch.int64, device="cuda")
    st = torch.full((M, nt, 2), 7.0, dtype=torch.float32, device="cuda") if lse else None
    out = torch.full((M, N), 3.0, dtype=BF16, device="cuda") if residual is None else residual.clone()
    ops.gemm(x, lin, out=out, argmax_partial=keys, lse_partial=st, sample=(temp, SEED, None) if temp else None,
             z13=True if kind == "z13" else None, residual=None if residual is None else out)
    return out, keys, st


@functools.lru_cache(maxsize=None)
def _case(kind, N, M, temp):
    """one GEMM with the statistics, shared by the tests that finish it"""
    return _gemm(kind, N, M, temp)


def _step_bufs(B, max_len, s=0):
    dev = "cuda"
    return dict(slot=torch.arange(10, 10 + B, dtype=torch.int32, device=dev), pos=torch.arange(20, 20 + B, dtype=torch.int32, device=dev),
                kvl=torch.arange(11, 11 + B, dtype=torch.int32, device=dev), ids=torch.full((B,), -5, dtype=torch.int64, device=dev),
                in_ids=torch.full((max_len, B), -7, dtype=torch.int64, device=dev),
                pred=torch.full((max_len, B), -9, dtype=torch.int64, device=dev),
                step=torch.full((B,), s, dtype=torch.int64, device=dev),
                lp=torch.full((max_len, B), 99.0, dtype=torch.float32, device=dev))


def _finish(logits, keys, st, temp, forced=None, max_len=2, s=0):
    ops = _ops()
    b = _step_bufs(keys.shape[0], max_len, s)
    ops.decode_step_end_logprob(b["slot"], b["pos"], b["kvl"], keys, st, b["ids"], b["in_ids"], b["pred"], b["step"], logits, b["lp"],
                                temperature=temp, forced_ids=forced)
    return b


# ----------------------------------------------------------------------------- 1. the epilogue's partials
@pytest.mark.parametrize("temp", [0.0, T_SAMPLE])
@pytest.mark.parametrize("N", [1000, 4112])       # 62 full tiles and one of 8 columns; 257 tiles
@pytest.mark.parametrize("kind", ["bf16", "fp8", "z13"])
def test_epilogue_partials(kind, N, temp):
    worst = 0.0
    for M in MS:
        logits, keys, st = _case(kind, N, M, temp)
        logits0, keys0, _ = _gemm(kind, N, M, temp, lse=False)
        assert _same(logits, logits0) and torch.equal(keys, keys0), f"M={M}: keys / logits changed by lse_partial"
        m, s = R.tile_stats(logits, temp)
        got = st.double().cpu()
        assert torch.equal(got[..., 0], m), f"M={M}: tile maxima"
        rel = ((got[..., 1] - s).abs() / s).max().item()
        worst = max(worst, rel)
        assert rel <= 1e-5, f"M={M}: s_t off by {rel:.3g} relative"
    print(f"epilogue partials {kind} N={N} T={temp}: largest relative error of s_t {worst:.3g}")


# ----------------------------------------------------------------------------- 2. the finished value
@pytest.mark.parametrize("temp", [0.0, T_SAMPLE])
@pytest.mark.parametrize("N", [1000, 4112])
@pytest.mark.parametrize("kind", ["bf16", "fp8", "z13"])
def test_finished_logprob(kind, N, temp):
    ops = _ops()
    worst = 0.0
    for M in MS:
        logits, keys, st = _case(kind, N, M, temp)
        b = _finish(logits, keys, st, temp)
        a = _step_bufs(M, 2)
        ops.decode_step_end_argmax(a["slot"], a["pos"], a["kvl"], keys, a["ids"], a["in_ids"], a["pred"], a["step"])
        for k in ("slot", "pos", "kvl", "ids", "in_ids", "pred", "step"):
            assert torch.equal(a[k], b[k]), f"M={M}: {k} differs from decode_step_end_argmax"
        if not temp:
            assert torch.equal(b["ids"].cpu(), logits.float().cpu().argmax(-1))       # (CPU argmax: lowest index on ties)
        want = R.logprob(logits, b["ids"], temp)
        err = (b["lp"][0].double().cpu() - want).abs().max().item()
        alone = ops.token_logprob(logits, b["ids"], temp)
        err2 = (alone.double().cpu() - want).abs().max().item()
        worst = max(worst, err, err2)
        assert want.abs().max() <= 200 and err <= BOUND and err2 <= BOUND, f"M={M}: fused {err:.3g}, stand-alone {err2:.3g}"
        assert (b["lp"][1] == 99.0).all()                 # only row s is written
    print(f"finished logprob {kind} N={N} T={temp}: largest |error| {worst:.3g}")


# ----------------------------------------------------------------------------- 3. -inf and NaN
@pytest.mark.parametrize("temp", [0.0, T_SAMPLE])
@pytest.mark.parametrize("kind", ["bf16", "fp8", "z13"])
def test_minus_inf_columns_and_nan(kind, temp):
    ops = _ops()
    N, M = 1000, 9
    logits, keys, st = _gemm(kind, N, M, temp, special="-inf")
    lc = logits.float().cpu()
    assert (lc[:, 32:48] == float("-inf")).all() and (lc[:, 100:104] == float("-inf")).all()
    g = st.cpu()
    assert not torch.isnan(g).any() and (g[:, 2, 0] == float("-inf")).all() and (g[:, 2, 1] == 0).all()
    m, s = R.tile_stats(logits, temp)
    assert torch.equal(g[..., 0].double(), m) and ((g[..., 1].double() - s).abs() <= 1e-5 * s).all()
    b = _finish(logits, keys, st, temp)
    want = R.logprob(logits, b["ids"], temp)
    got, alone = b["lp"][0].cpu(), ops.token_logprob(logits, b["ids"], temp).cpu()
    assert torch.isfinite(got).all() and torch.isfinite(alone).all()
    err = max((got.double() - want).abs().max().item(), (alone.double() - want).abs().max().item())
    print(f"-inf columns {kind} T={temp}: largest |error| {err:.3g}")
    assert err <= BOUND
    # the log-probability of a forced -inf token is -inf, not NaN
    forced = torch.full((2, M), 40, dtype=torch.int64, device="cuda")
    assert (_finish(logits, keys, st, temp, forced)["lp"][0] == float("-inf")).all()
    assert (ops.token_logprob(logits, forced[0].contiguous(), temp) == float("-inf")).all()
    # one NaN logit in row 4 (through the residual): that row is NaN in both kernels, the others are untouched
    res = torch.zeros((M, N), dtype=BF16, device="cuda")
    res[4, 517] = float("nan")
    logits, keys, st = _gemm(kind, N, M, temp, special="-inf", residual=res)
    assert torch.isnan(logits[4, 517]) and int(torch.isnan(logits.float()).sum()) == 1
    b = _finish(logits, keys, st, temp)
    alone = ops.token_logprob(logits, b["ids"], temp).cpu()
    got = b["lp"][0].cpu()
    others = [r for r in range(M) if r != 4]
    assert math.isnan(got[4]) and math.isnan(alone[4])
    want = R.logprob(logits, b["ids"], temp)
    assert (got[others].double() - want[others]).abs().max() <= BOUND and (alone[others].double() - want[others]).abs().max() <= BOUND


# ----------------------------------------------------------------------------- 4. the determinism rule
@pytest.mark.parametrize("temp", [0.0, T_SAMPLE])
@pytest.mark.parametrize("kind", ["bf16", "fp8", "z13"])
def test_bits_do_not_depend_on_the_batch(kind, temp):
    """row r alone (M = 1) and as row r of M = 8 and of M = 33: the same fp32 bits (statistics and finished value - of one forced
    token, since the sampler's draw, and so its pick, is keyed by the row index); the same call twice: the same bits"""
    N, r = 4112, 5
    x = _x()

    def run(M):
        xs = x[r:r + 1] if M == 1 else x[:M]
        logits, keys, st = _gemm(kind, N, M, temp, x=xs)
        forced = torch.full((2, M), 123, dtype=torch.int64, device="cuda")
        lp = _finish(logits, keys, st, temp, forced)["lp"][0]
        alone = _ops().token_logprob(logits, forced[0].contiguous(), temp)
        i = 0 if M == 1 else r
        return logits[i:i + 1], st[i:i + 1].clone(), lp[i:i + 1].clone(), alone[i:i + 1].clone(), keys, st
    one = run(1)
    for M in (8, 33):
        many, again = run(M), run(M)
        for a, b, what in zip(one[:4], many[:4], ("logits", "statistics", "logprob", "stand-alone logprob")):
            assert _same(a, b), f"row {r} alone vs in M={M}: {what} differ"
        assert torch.equal(many[4], again[4]) and _same(many[5], again[5]) and _same(many[2], again[2])


# ----------------------------------------------------------------------------- 5. forced tokens at kernel level
@pytest.mark.parametrize("temp", [0.0, T_SAMPLE])
def test_forced_tokens_kernel(temp):
    ops = _ops()
    N, B, L = 1000, 5, 4
    logits, keys, st = _case("bf16", N, 8, temp)
    logits, keys, st = logits[:B].contiguous(), keys[:B].contiguous(), st[:B].contiguous()
    forced = torch.full((L, B), -1, dtype=torch.int64)
    forced[:, 0] = torch.tensor([3, 999, 0, 517])          # always forced (the last column, the first, ...)
    forced[:, 2] = torch.tensor([-1, 42, -1, 7])           # mixed
    forced[:, 3] = torch.tensor([5, -1, -1, -1])
    forced[:, 4] = torch.tensor([-1, -1, -1, 88])
    forced = forced.cuda()
    b = _step_bufs(B, L)
    a = _step_bufs(B, L)
    pick = None
    for s in range(L):
        ops.decode_step_end_logprob(b["slot"], b["pos"], b["kvl"], keys, st, b["ids"], b["in_ids"], b["pred"], b["step"], logits, b["lp"],
                                    temperature=temp, forced_ids=forced)
        ops.decode_step_end_argmax(a["slot"], a["pos"], a["kvl"], keys, a["ids"], a["in_ids"], a["pred"], a["step"])
        pick = a["ids"].clone()
        fed = torch.where(forced[s] >= 0, forced[s], pick)
        assert torch.equal(b["ids"], fed) and torch.equal(b["pred"][s], pick)
        if s + 1 < L:
            assert torch.equal(b["in_ids"][s + 1], fed)
        want = R.logprob(logits, fed, temp)
        assert (b["lp"][s].double().cpu() - want).abs().max() <= BOUND
        for k in ("slot", "pos", "kvl", "step"):
            assert torch.equal(a[k], b[k]), k
    assert (b["in_ids"][0] == -7).all() and torch.equal(b["step"], torch.full((B,), L, dtype=torch.int64, device="cuda"))
    # past max_len nothing is logged, the counters still advance
    before = {k: v.clone() for k, v in b.items()}
    ops.decode_step_end_logprob(b["slot"], b["pos"], b["kvl"], keys, st, b["ids"], b["in_ids"], b["pred"], b["step"], logits, b["lp"],
                                temperature=temp, forced_ids=forced)
    for k in ("in_ids", "pred", "lp"):
        assert torch.equal(before[k], b[k])
    assert torch.equal(b["ids"], pick) and torch.equal(b["slot"], before["slot"] + 1) and torch.equal(b["step"], before["step"] + 1)


# ----------------------------------------------------------------------------- 5b. more tiles than one pass of the tile loops
V_MANY, PEAKS = 65560, (5, 16 * 2048 + 3, 65555)


@functools.lru_cache(maxsize=None)
def _many_tiles(temp):
    """4098 tiles: three passes of a 256-thread step end's walk over the keys (8 loads in flight: 2048 tiles a pass) and seventeen of
    its walks over the statistics, the last of each partial.  x = e_r, so row r's logits are column r of the weight: N(0, 2^2) and one
    logit 30 above the row maximum at PEAKS[r] - in tile 0, in the first tile of the second pass, in the last tile (8 columns)."""
    ops = _ops()
    Km, B, nt = 32, len(PEAKS), (V_MANY + 15) // 16
    w = torch.zeros((V_MANY, Km))
    w[:, :B] = torch.randn(V_MANY, B, generator=torch.Generator().manual_seed(V_MANY)) * 2
    for r, c in enumerate(PEAKS):
        w[c, r] = w[:, r].max() + 30
    x = torch.zeros((B, Km), dtype=BF16, device="cuda")
    x[torch.arange(B), torch.arange(B)] = 1.0
    keys = torch.zeros((B, nt), dtype=torch.int64, device="cuda")
    st = torch.full((B, nt, 2), 7.0, dtype=torch.float32, device="cuda")
    out = torch.full((B, V_MANY), 3.0, dtype=BF16, device="cuda")
    ops.gemm(x, ops.PackedLinear.from_weight(w.to(BF16).cuda()), out=out, argmax_partial=keys, lse_partial=st,
             sample=(temp, SEED, None) if temp else None)
    return out, keys, st


def _key_ids(keys):
    k = keys.cpu().numpy().view(np.uint64).max(axis=1)
    return torch.from_numpy((np.uint64(0xFFFFFFFF) - (k & np.uint64(0xFFFFFFFF))).astype(np.int64))


@pytest.mark.parametrize("temp", [0.0, T_SAMPLE])
def test_more_tiles_than_one_pass(temp):
    ops = _ops()
    logits, keys, st = _many_tiles(temp)
    B = len(PEAKS)
    want_ids = _key_ids(keys)                             # the host-side maximum over the keys
    if not temp:
        assert want_ids.tolist() == list(PEAKS)
    b = _finish(logits, keys, st, temp)
    a = _step_bufs(B, 2)
    ops.decode_step_end_argmax(a["slot"], a["pos"], a["kvl"], keys, a["ids"], a["in_ids"], a["pred"], a["step"])
    assert torch.equal(a["ids"].cpu(), want_ids) and torch.equal(b["ids"].cpu(), want_ids)
    for k in ("slot", "pos", "kvl", "in_ids", "pred", "step"):
        assert torch.equal(a[k], b[k]), k
    err = (b["lp"][0].double().cpu() - R.logprob(logits, b["ids"], temp)).abs().max().item()
    print(f"{(V_MANY + 15) // 16} tiles T={temp}: largest |error| {err:.3g}")
    assert err <= BOUND
    assert (b["lp"][1] == 99.0).all()                     # only row s is written


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


def _ctx(model, B=3):
    """a freshly prefilled cache of B text contexts and the start tokens"""
    from unimedvl_amd.kvcache import NaiveCache

    class Tok:
        def encode(self, s):
            return PROMPTS[int(s) % 3] + [int(s) // 3 + 5] * (int(s) // 3 > 0)
    cache = NaiveCache(model.cfg.layers)
    gi, kvl, rope = model.prepare_prompts([0] * B, [0] * B, [str(i) for i in range(B)], Tok(), NEW_TOKEN_IDS)
    cache = model.forward_cache_update_text(cache, **gi)
    return cache, model.prepare_start_tokens(kvl, rope, NEW_TOKEN_IDS)


def _session(model, steps=8, B=3, **kw):
    from unimedvl_amd.decode import DecodeSession
    cache, gi = _ctx(model, B)
    with torch.no_grad():
        return DecodeSession(model.language_model, cache, gi["packed_start_tokens"], gi["packed_query_position_ids"], steps, **kw)


def _kv(sess, steps):
    n = max(sess.lens0) + steps
    return [t[:, :, :n].clone() for s in sess.cache.slabs for t in (s.k,)] + [s.vt[:, :, :, :n].clone() for s in sess.cache.slabs]


SAMPLING = [dict(), dict(do_sample=True, temperature=T_SAMPLE, seed=77)]


# ----------------------------------------------------------------------------- 6. the session
@pytest.mark.parametrize("mode", SAMPLING, ids=["greedy", "sample"])
def test_session_logprobs(model, mode):
    steps = 8
    temp = mode.get("temperature", 0.0)
    with torch.no_grad():
        off = _session(model, steps, use_graph=True, **mode)
        off.step(steps)
        on = _session(model, steps, use_graph=True, logprobs=True, **mode)
        assert on.graph is not None and on.pred_logprobs.shape == (steps, 3) and on.pred_logprobs.dtype == torch.float32
        on.step(steps)
        assert torch.equal(on.pred_ids, off.pred_ids) and torch.equal(on.in_ids, off.in_ids)
        assert all(torch.equal(a, b) for a, b in zip(_kv(on, steps), _kv(off, steps)))
        eager = _session(model, steps, use_graph=False, logprobs=True, **mode)
        worst = 0.0
        for s in range(steps):
            eager.step(1)
            want = R.logprob(eager.logits, eager.pred_ids[s], temp)
            worst = max(worst, (eager.pred_logprobs[s].double().cpu() - want).abs().max().item())
        assert torch.equal(eager.pred_ids, on.pred_ids) and _same(eager.pred_logprobs, on.pred_logprobs)     # graph replay == eager
    print(f"session logprobs {mode}: largest |error| {worst:.3g}")
    assert worst <= BOUND
    # rewind_outputs starts at row 0 again
    on.rewind_outputs()
    assert int(on.step_idx.max()) == 0 and on.steps_done == 0


# ----------------------------------------------------------------------------- 7. forced session
def test_forced_session(model):
    steps = 8
    with torch.no_grad():
        free = _session(model, steps, use_graph=True, logprobs=True)
        free.step(steps)
        own = _session(model, steps, use_graph=True, forced_ids=free.pred_ids.cpu())
        assert own.logprobs and own.graph is not None
        own.step(steps)
        assert torch.equal(own.pred_ids, free.pred_ids) and torch.equal(own.in_ids, free.in_ids)
        assert _same(own.pred_logprobs, free.pred_logprobs)
        assert all(torch.equal(a, b) for a, b in zip(_kv(own, steps), _kv(free, steps)))
        # other tokens: exactly those are fed, and their value is the log-softmax of each step's logits
        g = torch.Generator().manual_seed(9)
        forced = torch.randint(5, 290, (steps, 3), generator=g)
        forced[2:5, 1] = -1                                # sample 1 runs free for three steps
        other = _session(model, steps, use_graph=False, forced_ids=forced)
        worst = 0.0
        for s in range(steps):
            other.step(1)
            fed = torch.where(forced[s] >= 0, forced[s], other.pred_ids[s].cpu())
            assert torch.equal(other.ids.cpu(), fed)
            if s + 1 < steps:
                assert torch.equal(other.in_ids[s + 1].cpu(), fed)
            assert torch.equal(other.pred_ids[s].cpu(), other.logits.float().cpu().argmax(-1))      # the model's own pick
            worst = max(worst, (other.pred_logprobs[s].double().cpu() - R.logprob(other.logits, fed)).abs().max().item())
        replay = _session(model, steps, use_graph=True, forced_ids=forced)
        replay.step(steps)
        assert _same(replay.pred_logprobs, other.pred_logprobs) and torch.equal(replay.in_ids, other.in_ids)
    print(f"forced session: largest |error| {worst:.3g}")
    assert worst <= BOUND
    with pytest.raises(ValueError, match="forced_ids"):
        _session(model, steps, forced_ids=torch.zeros((steps, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="vocab"):
        _session(model, steps, forced_ids=torch.full((steps, 3), model.cfg.vocab, dtype=torch.int64))


# ----------------------------------------------------------------------------- 8. generate_text
@pytest.mark.parametrize("eos", [None, "sample0", "per_sample"])
def test_generate_text_return_logprobs(model, eos):
    def run(**kw):
        cache, gi = _ctx(model)
        return model.generate_text(past_key_values=cache, max_length=8, **gi, **kw)
    base = run()
    kw = {}
    if eos is not None:       # stop on a token the greedy run emits at step 2 (sample 0) / somewhere for every sample
        kw = dict(end_token_id=int(base[3, 0]), per_sample_eos=eos == "per_sample")
    ids = run(**kw)
    ids2, lp = run(return_logprobs=True, **kw)
    assert torch.equal(ids, ids2) and lp.shape == (ids.shape[0], 3) and lp.dtype == torch.float32
    if eos == "sample0":
        assert ids.shape[0] <= 3
    ids3, logits, lp3 = run(return_logits=True, return_logprobs=True, **kw)
    assert torch.equal(ids3, ids) and logits.shape[0] == ids.shape[0] and _same(lp3, lp)           # eager == graph
    worst = 0.0
    for s in range(ids.shape[0]):
        tok = ids[s + 1] if s + 1 < ids.shape[0] else logits[s].float().cpu().argmax(-1)
        worst = max(worst, (lp[s].double().cpu() - R.logprob(logits[s], tok)).abs().max().item())
    print(f"generate_text eos={eos}: rows {ids.shape[0]}, largest |error| {worst:.3g}")
    assert worst <= BOUND
    # sampling: reproducible under torch.manual_seed, the value is that of softmax(bf16(logits / T))
    torch.manual_seed(3)
    a, la = run(do_sample=True, temperature=T_SAMPLE, return_logprobs=True, **kw)
    torch.manual_seed(3)
    b, logits, lb = run(do_sample=True, temperature=T_SAMPLE, return_logits=True, return_logprobs=True, **kw)
    torch.manual_seed(3)
    assert torch.equal(a, run(do_sample=True, temperature=T_SAMPLE, **kw))
    assert torch.equal(a, b) and _same(la, lb)
    for s in range(a.shape[0] - 1):
        assert (la[s].double().cpu() - R.logprob(logits[s], a[s + 1], T_SAMPLE)).abs().max() <= BOUND
    out, lp0 = model.generate_text(past_key_values=_ctx(model)[0], max_length=0, return_logprobs=True, **_ctx(model)[1])
    assert out.shape == (0, 3) and lp0.shape == (0, 3)


# ----------------------------------------------------------------------------- 9. Bagel.score
def test_score(model):
    from oracle.toy_tokenizer import ToyTokenizer
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    ident = lambda x: x   # noqa: E731
    img = torch.randn(3, 28, 42, generator=torch.Generator().manual_seed(2)).clamp(-1, 1)
    prompt = "17 23 5"
    answer, own, own_lp = model.chat(tok, NEW_TOKEN_IDS, ident, [img], prompt, max_length=6, return_logprobs=True)
    assert answer == model.chat(tok, NEW_TOKEN_IDS, ident, [img], prompt, max_length=6) and len(own) == len(own_lp) >= 1
    cands = [own, [7, 8], [9, 10, 11, 12, 13, 14, 15]]
    res = model.score(tok, NEW_TOKEN_IDS, ident, [img], prompt, cands)
    assert len(res) == 3
    eos = NEW_TOKEN_IDS["eos_token_id"]
    for c, r in zip(cands, res):
        assert r["token_ids"] == list(c) + [eos] and len(r["token_logprobs"]) == len(c) + 1
        assert r["logprob"] == float(torch.tensor(r["token_logprobs"], dtype=torch.float64).sum())
        assert all(math.isfinite(v) and v <= 0 for v in r["token_logprobs"])
    # batch independence: the same values as the request decoded on its own (3 rows against 1), bit for bit
    assert res[0]["token_logprobs"][:len(own)] == own_lp
    # strings go through tokenizer.encode; without the end token only the candidate's own tokens are scored
    as_text = model.score(tok, NEW_TOKEN_IDS, ident, [img], prompt, [" ".join(str(t) for t in c) for c in cands])
    assert as_text == res
    bare = model.score(tok, NEW_TOKEN_IDS, ident, [img], prompt, cands, append_eos=False)
    for b, r in zip(bare, res):
        assert b["token_ids"] == r["token_ids"][:-1] and b["token_logprobs"] == r["token_logprobs"][:-1]
    with pytest.raises(ValueError, match="64"):
        model.score(tok, NEW_TOKEN_IDS, ident, [img], prompt, [[7]] * 65)


# ----------------------------------------------------------------------------- 10. the batcher
def _requests(n):
    g = torch.Generator().manual_seed(21)
    reqs = []
    for i in range(n):
        h, w = [(42, 56), (28, 70), (56, 56), (42, 42)][i % 4]
        images = [] if i % 5 == 4 else [torch.randn(3, h, w, generator=g).clamp(-1, 1)]
        if i % 7 == 3:
            images.append(torch.randn(3, 28, 28, generator=g).clamp(-1, 1))
        prompt = " ".join(str(int(v)) for v in torch.randint(5, 290, (2 + i % 6,), generator=g))
        reqs.append((images, prompt))
    return reqs


@pytest.mark.parametrize("paged", [False, True], ids=["slab", "paged"])
def test_batcher_logprobs(model, paged):
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.serving import ContinuousBatcher
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    reqs = _requests(7)
    budgets = [6, 3, 6, 5, 6, 2, 6]
    ident = lambda x: x   # noqa: E731

    def serve(**kw):
        srv = ContinuousBatcher(model, tok, NEW_TOKEN_IDS, ident, slots=3, max_context=256, max_new_tokens=8, check_every=4,
                                paged=paged, **kw)
        rids = [srv.submit(images, prompt, max_new_tokens=nb) for (images, prompt), nb in zip(reqs, budgets)]
        return srv, rids, srv.run()
    _, rids0, plain = serve()
    srv, rids, got = serve(logprobs=True)
    assert rids == rids0 and got == plain and sorted(srv.logprobs) == sorted(rids)
    for rid, (images, prompt), nb in zip(rids, reqs, budgets):
        answer, toks, lps = model.chat(tok, NEW_TOKEN_IDS, ident, images, prompt, max_length=nb + 1, return_logprobs=True)
        assert got[rid] == answer and len(toks) <= nb
        assert len(srv.logprobs[rid]) == len(toks), rid
        assert srv.logprobs[rid] == lps, rid                 # bit for bit: a request's values do not depend on its neighbours


# ----------------------------------------------------------------------------- 11. refusals
def test_refusals(model, monkeypatch):
    ops = _ops()
    from unimedvl_amd import _lib
    with monkeypatch.context() as mp:
        mp.setenv("UMV_DECODE_FUSED_ARGMAX", "0")
        with pytest.raises(ValueError, match="UMV_DECODE_FUSED_ARGMAX"):
            _session(model, 4, use_graph=False, logprobs=True)
        assert _session(model, 4, use_graph=False).fused_argmax is False
    with pytest.raises(ValueError, match="64 samples"):
        _session(model, 2, B=65, use_graph=False, logprobs=True)
    lin = _lin("bf16", 1000)
    st = torch.zeros((8, 63, 2), dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.UmvError, match=r"rc=-1\b.*lse_partial"):          # UMV_ERR_ARG
        ops.gemm(_x()[:8], lin, lse_partial=st)
    with pytest.raises(_lib.UmvError, match="lse_partial"):
        ops.gemm(_x()[:8], lin, argmax_partial=torch.zeros((8, 63), dtype=torch.int64, device="cuda"), lse_partial=st[:, :10])
