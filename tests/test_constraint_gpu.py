"""umv_logit_constrain_bf16 and umv_constraint_advance (include/unimedvl_hip.h, "token automata") at kernel level: the masked logits
against the numpy model of the definition (tests/constraint_ref.py), the recomputed tiles against the lm_head epilogue itself (a
fully-allowed state: nothing may move), against the shared tile recomputation run over every tile of the model's masked row (the
penalty kernel with neutral parameters and one list entry per tile: bit for bit, greedy and sampled, keys and statistics - this is
what pins the no-load shortcut of a tile without an allowed column) and against the model's tiles; the picks of the fused step ends
against the stand-alone entries on the masked logits; the state words against `walk`; batch independence; the sampling distribution.

Everything is asserted bit for bit, with the exceptions the header already bounds: a log-probability against umv_token_logprob_bf16
and against the fp64 restricted log-softmax is within the header's 1e-4.  A tile's sum of exponentials against the fp64 model: 16
terms, each a fast fp32 exponential of a bf16-exact difference (relative error of the hardware exp2 path below 2^-21), summed in a
tree of four fp32 roundings: 1e-5 relative is well above what that can add up to."""
import functools

import numpy as np
import pytest
import torch

import constraint_ref as C
import penalty_ref as P

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
T = 0.7
SEED = 4321
K = 512
BOUND = 1e-4          # of a log-probability (include/unimedvl_hip.h, token log-probabilities; tests/logprob_ref.py)
SUM_RTOL = 1e-5       # of a tile's sum of exponentials against fp64 (the module docstring)
MODES = [(0.0, False), (0.0, True), (T, False), (T, True)]        # (temperature: 0 = greedy, with lse_partial)
NINF, NAN = 0xFF80, 0x7FC0


def _ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd import ops
    return ops


CH = __import__("unimedvl_amd.ops", fromlist=["CONSTRAIN_CHUNK"]).CONSTRAIN_CHUNK     # the columns one workgroup masks
VS = [40, 330, CH + 16 * 3 + 8]      # last tile partial; 330; two chunks per row and a partial last tile


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _from_bits(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(BF16)


def _eq_stats(a, b):
    a, b = a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32)
    fa, fb = a.view(np.float32), b.view(np.float32)
    return ((a == b) | (np.isnan(fa) & np.isnan(fb))).all()


@functools.lru_cache(maxsize=None)
def _problem(M, V):
    """x [M, K] and the packed lm_head weight [V, K] on the device: logits ~ N(0, 3^2)"""
    ops = _ops()
    g = torch.Generator().manual_seed(100 * M + V)
    x = torch.randn(M, K, generator=g).to(BF16).cuda()
    w = (torch.randn(V, K, generator=g) * (3.0 / K ** 0.5)).to(BF16).cuda()
    return x, ops.PackedLinear.from_weight(w)


def _lm_head(x, lin, temp, lse, step=None, rows=None):
    """the lm_head call: (logits with a row stride beyond V, argmax_partial, lse_partial or None)"""
    ops = _ops()
    M, V = x.shape[0], lin.N
    nt = (V + 15) // 16
    out = torch.empty((M, (V + 7) // 8 * 8 + 8), dtype=BF16, device="cuda")[:, :V]
    keys = torch.zeros((M, nt), dtype=torch.int64, device="cuda")
    stats = torch.full((M, nt, 2), 55.0, dtype=torch.float32, device="cuda") if lse else None
    if rows is not None:
        ops.gemm(x, lin, out=out, argmax_partial=keys, lse_partial=stats, sample_rows=rows)
    else:
        ops.gemm(x, lin, out=out, argmax_partial=keys, lse_partial=stats, sample=(temp, SEED, step) if temp > 0 else None)
    return out, keys, stats


# ----------------------------------------------------------------------------- the automaton of the cases
FULL, EMPTY, TWELVE = 2, 4, 6


@functools.lru_cache(maxsize=None)
def _automaton(V):
    """state 0: one edge; 1: columns 0 and V - 1 (the partial tile); 2: every column; 3: one column and two edge tokens >= V (ignored);
    4: no edge; 5: with two chunks the last tile of chunk 0 and the first of chunk 1, else the partial tile and its neighbour;
    6: twelve columns, two of them neighbours in one tile."""
    if V > CH:
        five = [CH - 16, CH - 1, CH, CH + 15, V - 3]
    else:
        five = [V - 2, V - 3, (V - 1) // 16 * 16 - 1, 17]
    rng = np.random.default_rng(V)
    twelve = rng.choice([n for n in range(V) if n not in (20, 21)], size=10, replace=False).tolist() + [20, 21]
    states = [[(V // 2, 1)], [(0, 2), (V - 1, 0)], [(n, 2) for n in range(V)], [(5, 3), (V, 0), (V + 100, 1)], [],
              [(n, 6) for n in sorted(set(five))], [(n, 6 if n % 2 else -1) for n in sorted(set(twelve))]]
    ref = C.Automaton.from_states(states)
    from unimedvl_amd.constraints import TokenAutomaton
    host = TokenAutomaton(*ref.arrays(), allow_empty_states=True)
    return ref, host, host.to_device("cuda")


def _row_states(M, n_states):
    """masked and free rows interleaved: -1, -2 and a word >= n_states between the seven states"""
    cycle = [0, 1, -1, 2, 3, -2, 4, 5, n_states + 1, 6]
    return [cycle[m % len(cycle)] for m in range(M)] if M > 1 else [5]


def _all_tiles_through_penalty_tile(logits, temp, lse, step=None, rows=None):
    """keys and statistics of EVERY tile of `logits` as the shared tile recomputation leaves them: the penalty kernel with neutral
    parameters, an id nothing records and a visit list that names one column of every tile"""
    ops = _ops()
    M, V = logits.shape
    nt = (V + 15) // 16
    keys = torch.zeros((M, nt), dtype=torch.int64, device="cuda")
    stats = torch.full((M, nt, 2), 55.0, dtype=torch.float32, device="cuda") if lse else None
    lst = (torch.arange(nt, dtype=torch.int32, device="cuda") * 16).repeat(M, 1).contiguous()
    before = logits.clone()
    ops.logit_penalty(logits, torch.full((M,), -1, dtype=torch.int64, device="cuda"), torch.zeros((M, V), dtype=torch.int32, device="cuda"),
                      lst, torch.full((M,), nt, dtype=torch.int32, device="cuda"), nt, temperature=0.0 if rows is not None else temp,
                      seed=SEED, step=step, argmax_partial=keys, lse_partial=stats, sample_rows=rows)
    assert torch.equal(before.view(torch.int16), logits.view(torch.int16)), "the neutral penalty call must leave the logits"
    return keys, stats


def _check_tiles_against_model(masked_bits, keys, stats, temp, what):
    """one row: greedy keys exact, statistics against fp64 (maximum exact, sum within SUM_RTOL)"""
    if temp == 0:
        assert np.array_equal(keys.cpu().numpy().view(np.uint64), P.greedy_keys(masked_bits)), f"{what}: greedy keys against the model"
    if stats is not None:
        m, s = P.tile_stats(masked_bits, temp)
        got = stats.cpu().numpy().astype(np.float64)
        ok_m = (got[:, 0] == m) | (np.isnan(got[:, 0]) & np.isnan(m))
        ok_s = (np.abs(got[:, 1] - s) <= SUM_RTOL * np.abs(s)) | (np.isnan(got[:, 1]) & np.isnan(s))
        assert ok_m.all() and ok_s.all(), f"{what}: statistics against the fp64 model, tiles {np.flatnonzero(~(ok_m & ok_s))[:6]}"


# ----------------------------------------------------------------------------- 1. against the lm_head epilogue and the model
@pytest.mark.parametrize("M", [1, 8, 64])
@pytest.mark.parametrize("V", VS)
def test_masked_rows_against_the_epilogue_and_the_model(V, M):
    ops = _ops()
    ref, _, dev = _automaton(V)
    states = _row_states(M, ref.n_states) if M > 1 else [FULL]
    state = torch.tensor(states, dtype=torch.int32, device="cuda")
    masked_rows = [m for m, s in enumerate(states) if not ref.free(s)]
    x, lin = _problem(M, V)
    step = torch.tensor([3], dtype=torch.int64, device="cuda")
    for temp, lse in MODES:
        out, keys, stats = _lm_head(x, lin, temp, lse, step)
        raw = _bits(out)
        want = (out.clone(), keys.clone(), stats.clone() if lse else None)
        at = torch.tensor(masked_rows, device="cuda")
        keys[at] = 0                                   # poison what the kernel must write: every tile of a masked row
        if lse:
            stats[at] = 55.0
        ops.logit_constrain(out, dev, state, temperature=temp, seed=SEED, step=step, argmax_partial=keys, lse_partial=stats)
        assert torch.equal(state.cpu(), torch.tensor(states, dtype=torch.int32)), "the mask kernel only reads the state words"
        got = _bits(out)
        model = np.stack([C.mask_row(raw[m], ref, s) for m, s in enumerate(states)])
        assert np.array_equal(got, model), f"T={temp}: masked logits, rows {np.flatnonzero((got != model).any(1))[:6]}"
        tk, ts = _all_tiles_through_penalty_tile(_from_bits(model).cuda(), temp, lse, step)
        for m, s in enumerate(states):
            tag = f"V={V} M={M} T={temp} lse={lse} row {m} state {s}"
            if ref.free(s) or s == FULL:               # a free row is not touched; a fully-allowed one is rewritten with the epilogue's own bits
                assert torch.equal(out[m].view(torch.int16), want[0][m].view(torch.int16)), tag
                assert torch.equal(keys[m], want[1][m]), f"{tag}: keys are not the lm_head epilogue's"
                assert not lse or _eq_stats(stats[m], want[2][m]), f"{tag}: statistics are not the lm_head epilogue's bits"
                continue
            assert torch.equal(keys[m], tk[m]), f"{tag}: keys differ from the shared tile recomputation's"
            assert not lse or _eq_stats(stats[m], ts[m]), f"{tag}: statistics differ from the shared tile recomputation's"
            _check_tiles_against_model(model[m], keys[m], stats[m] if lse else None, temp, tag)
            if s == EMPTY and lse:
                assert (stats[m, :, 0] == float("-inf")).all() and (stats[m, :, 1] == 0).all()


# ----------------------------------------------------------------------------- 2. crafted rows, aligned and unaligned row strides
def _crafted(V):
    """(name, row bits, state): ties inside the allowed set, -inf and NaN inside and outside it"""
    ref, _, _ = _automaton(V)
    rng = np.random.default_rng(V + 1)
    base = P.bf16_bits((rng.standard_normal(V) * 3).astype(np.float32))
    six = ref.allowed(TWELVE, V)
    five = ref.allowed(5, V)
    cases = [("random", base.copy(), 0), ("random", base.copy(), 1), ("random", base.copy(), 5), ("every column", base.copy(), FULL),
             ("tokens >= V", base.copy(), 3), ("empty", base.copy(), EMPTY), ("free -1", base.copy(), -1), ("free -2", base.copy(), -2),
             ("free beyond", base.copy(), ref.n_states)]
    b = base.copy()
    b[six] = P.bf16_bits(np.array([2.5], dtype=np.float32))[0]              # every allowed column tied
    cases.append(("tied", b, TWELVE))
    b = base.copy()
    b[six[:6]] = NINF                                                       # -inf inside A ...
    b[[n for n in range(V) if n not in six][:5]] = NINF                     # ... and outside
    cases.append(("-inf", b, TWELVE))
    b = base.copy()
    b[six] = NINF                                                           # A holds -inf only: the row of -inf
    cases.append(("all -inf", b, TWELVE))
    b = base.copy()
    b[six[3]] = NAN                                                         # NaN inside A keeps its bits
    b[six[4]] = 0xFFC1                                                      # (a negative NaN with a payload too)
    cases.append(("NaN inside", b, TWELVE))
    b = base.copy()
    b[[n for n in range(V) if n not in five][:3]] = NAN                     # NaN outside A becomes -inf
    b[V - 1 if V - 1 not in five else V - 4] = NAN
    cases.append(("NaN outside", b, 5))
    b = base.copy()
    b[0], b[V - 1], b[1], b[2] = 0x8000, 0x0000, NAN, NINF                  # -0 and +0 tied across the row's ends
    cases.append(("zeros", b, 1))
    return cases


@pytest.mark.parametrize("pad", [8, 3])          # row stride V + pad: 16-byte aligned rows (V + 8 with V % 8 == 0), or the scalar path
@pytest.mark.parametrize("V", VS)
def test_crafted_rows(V, pad):
    ops = _ops()
    ref, _, dev = _automaton(V)
    cases = _crafted(V)
    M = len(cases)
    bits = np.stack([c[1] for c in cases])
    states = [c[2] for c in cases]
    state = torch.tensor(states, dtype=torch.int32, device="cuda")
    model = np.stack([C.mask_row(bits[m], ref, s) for m, s in enumerate(states)])
    nt = (V + 15) // 16
    step = torch.tensor([5], dtype=torch.int64, device="cuda")
    for temp, lse in MODES:
        buf = torch.full((M, V + pad), 7.0, dtype=BF16, device="cuda")
        buf[:, :V] = _from_bits(bits).cuda()
        logits = buf[:, :V]
        keys = torch.full((M, nt), 77, dtype=torch.int64, device="cuda")
        stats = torch.full((M, nt, 2), 55.0, dtype=torch.float32, device="cuda") if lse else None
        ops.logit_constrain(logits, dev, state, temperature=temp, seed=SEED, step=step, argmax_partial=keys, lse_partial=stats)
        got = _bits(logits)
        assert np.array_equal(got, model), f"pad={pad} T={temp}: rows {[cases[m][0] for m in np.flatnonzero((got != model).any(1))]}"
        assert (buf[:, V:] == 7.0).all(), "the columns behind V were written"
        tk, ts = _all_tiles_through_penalty_tile(_from_bits(model).cuda(), temp, lse, step)
        for m, (name, _, s) in enumerate(cases):
            if ref.free(s):
                assert (keys[m] == 77).all() and (not lse or (stats[m] == 55.0).all()), f"{name}: a free row's tiles were written"
                continue
            assert torch.equal(keys[m], tk[m]), f"{name} pad={pad} T={temp}: keys"
            assert not lse or _eq_stats(stats[m], ts[m]), f"{name} pad={pad} T={temp}: statistics"
            _check_tiles_against_model(model[m], keys[m], stats[m] if lse else None, temp, name)
    # the unfused use: no partials, the logits only
    logits = _from_bits(bits).cuda()
    ops.logit_constrain(logits, dev, state)
    assert np.array_equal(_bits(logits), model)


# ----------------------------------------------------------------------------- 3. picks against the independent entries
def _step_bufs(B, max_len, s):
    dev = "cuda"
    return dict(slot=torch.zeros(B, dtype=torch.int32, device=dev), pos=torch.zeros(B, dtype=torch.int32, device=dev),
                kvl=torch.ones(B, dtype=torch.int32, device=dev), ids=torch.full((B,), -5, dtype=torch.int64, device=dev),
                in_ids=torch.zeros((max_len, B), dtype=torch.int64, device=dev), pred=torch.zeros((max_len, B), dtype=torch.int64, device=dev),
                step=torch.full((B,), s, dtype=torch.int64, device=dev), lp=torch.zeros((max_len, B), dtype=torch.float32, device=dev),
                cut=torch.zeros((max_len, B), dtype=torch.float32, device=dev), kept=torch.zeros((max_len, B), dtype=torch.int32, device=dev))


def _constrained(M, V, temp, lse, s=2, rows=None):
    """lm_head call, then the mask: (raw bits, masked logits, keys, stats, step buffers, the rows' states)"""
    ops = _ops()
    ref, _, dev = _automaton(V)
    states = _row_states(M, ref.n_states)
    x, lin = _problem(M, V)
    b = _step_bufs(M, 4, s)
    out, keys, stats = _lm_head(x, lin, temp, lse, b["step"], rows)
    raw = _bits(out)
    ops.logit_constrain(out, dev, torch.tensor(states, dtype=torch.int32, device="cuda"), temperature=0.0 if rows is not None else temp,
                        seed=SEED, step=b["step"], argmax_partial=keys, lse_partial=stats, sample_rows=rows)
    return raw, out, keys, stats, b, states


def _drawable(states, ref, V):
    """rows a sampled pick is compared on: all but those in the empty state.  Their masked row is -inf only, and for such a row the
    stand-alone samplers report no column (umv_sample_bf16 leaves 0x7FFFFFFF) where the fused step ends report column 0: the two
    entries differ there whatever produced the row, so there is nothing of this kernel's to compare.  The greedy pick is compared."""
    return torch.tensor([ref.allowed(s, V) != [] for s in states], device="cuda")


def _in_allowed_set(ids, states, ref, V):
    for m, (i, s) in enumerate(zip(ids.tolist(), states)):
        A = ref.allowed(s, V)
        assert A is None or not A or i in A, f"row {m} in state {s} picked {i}, outside {A[:8]}"


def _check_logprobs(lp, alone, raw, ids, states, ref, V, temp, what):
    """the fused step end's log-probabilities against the stand-alone entry on the masked logits and against the fp64 log-softmax
    restricted to the allowed set of the RAW row (an empty set has none: a row of -inf only has no finite log-probability)"""
    lp, alone = lp.cpu().double(), alone.cpu().double()
    worst = 0.0
    for m, s in enumerate(states):
        A = ref.allowed(s, V)
        if A is not None and not A:
            assert not bool(torch.isfinite(lp[m])) and not bool(torch.isfinite(alone[m])), f"row {m}: a finite log-probability on a row of -inf"
            continue
        model = P.logprob(raw[m], int(ids[m]), temp) if A is None else C.restricted_logprob(raw[m], A, int(ids[m]), temp)
        worst = max(worst, abs(float(lp[m]) - float(alone[m])), abs(float(lp[m]) - model))
    print(f"{what}: log-probability off the stand-alone entry / the fp64 restricted log-softmax by at most {worst:.3g}")
    assert worst <= BOUND, what


@pytest.mark.parametrize("M", [1, 8, 64])
@pytest.mark.parametrize("V", VS)
def test_fused_picks_equal_the_stand_alone_entries_on_the_masked_logits(V, M):
    ops = _ops()
    ref = _automaton(V)[0]
    s = 2
    # greedy: umv_decode_step_end_argmax against umv_argmax_bf16
    raw, out, keys, _, b, states = _constrained(M, V, 0.0, False, s)
    ops.decode_step_end_argmax(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"])
    assert torch.equal(b["ids"], ops.argmax(out)), "greedy"
    _in_allowed_set(b["ids"], states, ref, V)
    for m, st in enumerate(states):
        A = ref.allowed(st, V)
        if A:
            assert int(b["ids"][m]) == C.restricted_argmax(raw[m], A), f"row {m}: not the lowest-column argmax over the allowed set"
    # greedy log-probability: umv_decode_step_end_logprob against umv_token_logprob_bf16 and the fp64 model
    raw, out, keys, stats, b, states = _constrained(M, V, 0.0, True, s)
    ops.decode_step_end_logprob(b["slot"], b["pos"], b["kvl"], keys, stats, b["ids"], b["in_ids"], b["pred"], b["step"], out, b["lp"], 0.0)
    _check_logprobs(b["lp"][s], ops.token_logprob(out, b["ids"], 0.0), raw, b["ids"], states, ref, V, 0.0, f"V={V} M={M} greedy")
    # sampling: the step end on the sampling keys against umv_sample_bf16 with the same (seed, step)
    raw, out, keys, _, b, states = _constrained(M, V, T, False, s)
    st = b["step"][:1].clone()
    ops.decode_step_end_argmax(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"])
    ok = _drawable(states, ref, V)
    assert torch.equal(b["ids"][ok], ops.sample(out, T, SEED, step=st)[ok]), "sampling"
    _in_allowed_set(b["ids"], states, ref, V)
    # truncated sampling (with log-probabilities): umv_decode_step_end_truncated against umv_sample_truncated_bf16
    raw, out, keys, stats, b, states = _constrained(M, V, T, True, s)
    flt = dict(top_k=5, top_p=0.8)
    cut = torch.zeros(M, dtype=torch.float32, device="cuda")
    kept = torch.zeros(M, dtype=torch.int32, device="cuda")
    alone = ops.sample_truncated(out, T, SEED, step=b["step"][:1].clone(), cut_y=cut, n_kept=kept, **flt)
    ops.decode_step_end_truncated(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"], out, T, SEED,
                                  lse_partial=stats, logprobs=b["lp"], cut_y=b["cut"], n_kept=b["kept"], **flt)
    assert torch.equal(b["ids"][ok], alone[ok]), "truncated: ids"
    assert torch.equal(b["cut"][s].view(torch.int32), cut.view(torch.int32)) and torch.equal(b["kept"][s], kept), "truncated: cutoff"
    _in_allowed_set(b["ids"], states, ref, V)
    _check_logprobs(b["lp"][s], ops.token_logprob(out, b["ids"], T), raw, b["ids"], states, ref, V, T, f"V={V} M={M} truncated")


@pytest.mark.parametrize("M", [1, 8, 64])
@pytest.mark.parametrize("V", VS)
def test_rows_step_end_on_the_recomputed_partials(V, M):
    """a per-row table: even rows sample with filters, odd rows are greedy; every row keyed (SEED, draw = the step, stream = the row) -
    the scalar calls' keying, so the stand-alone scalar entries name the same draws"""
    ops = _ops()
    from unimedvl_amd import sampling
    ref = _automaton(V)[0]
    s = 2
    flt = dict(top_k=5, top_p=0.8)
    params = [sampling.SamplingParams(do_sample=True, temperature=T, **flt) if m % 2 == 0 else sampling.SamplingParams() for m in range(M)]
    table = sampling.to_tensor(sampling.pack(params, seed=SEED, streams=list(range(M)), draws=[s] * M), "cuda")
    raw, out, keys, stats, b, states = _constrained(M, V, 0.0, True, s, rows=table)
    tk, ts = _all_tiles_through_penalty_tile(out.clone(), 0.0, True, rows=table)
    for m, st in enumerate(states):
        if not ref.free(st):
            assert torch.equal(keys[m], tk[m]) and _eq_stats(stats[m], ts[m]), f"row {m}: tiles under the row's own temperature and key"
    ops.decode_step_end_rows(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"], out, table, lse_partial=stats,
                             logprobs=b["lp"], cut_y=b["cut"], n_kept=b["kept"])
    sampled = ops.sample_truncated(out, T, SEED, step=torch.tensor([s], dtype=torch.int64, device="cuda"), **flt)
    greedy = ops.argmax(out)
    even = torch.arange(M, device="cuda") % 2 == 0
    ok = _drawable(states, ref, V) | ~even
    assert torch.equal(b["ids"][ok], torch.where(even, sampled, greedy)[ok]), "ids against the scalar stand-alone entries"
    _in_allowed_set(b["ids"], states, ref, V)
    lp_alone = torch.where(even, ops.token_logprob(out, b["ids"], T), ops.token_logprob(out, b["ids"], 0.0))
    for sel, temp in ((even, T), (~even, 0.0)):
        idx = torch.nonzero(sel).flatten().tolist()
        if idx:
            _check_logprobs(b["lp"][s][idx], lp_alone[idx], raw[idx], b["ids"][idx], [states[m] for m in idx], ref, V, temp, f"V={V} M={M} rows T={temp}")


# ----------------------------------------------------------------------------- 4. the advance kernel
@pytest.mark.parametrize("M", [1, 8, 64])
def test_advance_follows_walk(M):
    ops = _ops()
    from unimedvl_amd.constraints import FREE, LEFT, TokenAutomaton
    eos = 3
    members = {"abcd": TokenAutomaton.from_choices([[10, 11, 12], [10, 11], [10, 13, 14, 15], [20]], eos),
               "set": TokenAutomaton.from_allowed_tokens([5, 7, 9, 200000]),
               "prefix": TokenAutomaton.from_choices([[30, 31, 32]], None, after="free")}
    host, start = TokenAutomaton.union(members)
    dev = host.to_device("cuda")
    rng = np.random.default_rng(M)
    names = list(members)
    s0 = [[start[names[m % 3]], FREE, LEFT, host.n_states + 5][m % 4] if m % 5 == 4 else start[names[m % 3]] for m in range(M)]
    state = torch.tensor(s0, dtype=torch.int32, device="cuda")
    guard = torch.full((M + 2,), -99, dtype=torch.int32, device="cuda")
    guard[1:M + 1] = state
    state = guard[1:M + 1]
    cur = list(s0)
    for step in range(6):
        ids = []
        for m in range(M):
            A = host.allowed(cur[m])
            if A is None or (m % 7 == 3 and step == 2):
                ids.append(int(rng.integers(0, 300000)) if m % 2 else 4)           # a forced foreign token (4 has no edge anywhere)
            else:
                ids.append(int(A[int(rng.integers(0, len(A)))]))
        ops.constraint_advance(dev, state, torch.tensor(ids, dtype=torch.int64, device="cuda"))
        cur = [host.walk(c, [t]) for c, t in zip(cur, ids)]
        assert state.cpu().tolist() == cur, f"step {step}"
        assert int(guard[0]) == -99 and int(guard[-1]) == -99, "a word outside state [M] was written"
    assert M < 8 or LEFT in cur, "the walk never left: the foreign-token case did not run"
    assert all(c == s for c, s in zip(cur, s0) if s < 0 or s >= host.n_states), "a free row's word moved"
    # an id beyond int32 has no edge
    st = torch.tensor([start["set"]], dtype=torch.int32, device="cuda")
    ops.constraint_advance(dev, st, torch.tensor([(1 << 32) + 5], dtype=torch.int64, device="cuda"))
    assert int(st[0]) == LEFT


# ----------------------------------------------------------------------------- 5. batch independence
@pytest.mark.parametrize("V", [330, VS[2]])
def test_a_row_does_not_depend_on_its_batch(V):
    """a row alone and as one of 8 or 33: the same logits, keys and statistics.  (The scalar sampling key names the row index, so the
    sampled comparison is the one of row 0; greedy rows are compared wherever they sit.)"""
    ops = _ops()
    ref, _, dev = _automaton(V)
    step = torch.tensor([1], dtype=torch.int64, device="cuda")
    for M in (8, 33):
        x, lin = _problem(M, V)
        states = [(5, 6, 1, 3, 0, 4)[m % 6] for m in range(M)]
        for temp in (0.0, T):
            out, keys, stats = _lm_head(x, lin, temp, True, step)
            ops.logit_constrain(out, dev, torch.tensor(states, dtype=torch.int32, device="cuda"), temperature=temp, seed=SEED, step=step,
                                argmax_partial=keys, lse_partial=stats)
            for i in ((0, 5, M - 1) if temp == 0 else (0,)):
                o1, k1, s1 = _lm_head(x[i:i + 1].contiguous(), lin, temp, True, step)
                ops.logit_constrain(o1, dev, torch.tensor(states[i:i + 1], dtype=torch.int32, device="cuda"), temperature=temp, seed=SEED,
                                    step=step, argmax_partial=k1, lse_partial=s1)
                assert torch.equal(o1.view(torch.int16), out[i:i + 1].view(torch.int16)) and torch.equal(k1, keys[i:i + 1]) \
                    and _eq_stats(s1, stats[i:i + 1]), f"row {i} of {M} T={temp}"


# ----------------------------------------------------------------------------- 6. the sampling distribution
def test_draws_follow_the_softmax_renormalised_over_the_allowed_set():
    """16 384 draws of one masked row with the stand-alone sampler over varying step: no draw outside the 12-token set, frequencies
    within chi2 < dof + 6 sqrt(2 dof) over the cells with expectation > 5 (the bound of the project's sampler tests)"""
    ops = _ops()
    V, N = 330, 16384
    ref, _, dev = _automaton(V)
    A = ref.allowed(TWELVE, V)
    assert len(A) == 12
    rng = np.random.default_rng(12)
    bits = P.bf16_bits((rng.standard_normal(V) * 2).astype(np.float32))
    logits = _from_bits(bits).reshape(1, V).cuda()
    ops.logit_constrain(logits, dev, torch.tensor([TWELVE], dtype=torch.int32, device="cuda"))
    draws = torch.full((N,), -1, dtype=torch.int64, device="cuda")
    steps = torch.arange(N, dtype=torch.int64, device="cuda")
    for i in range(N):
        ops.sample(logits, T, SEED, step=steps[i:i + 1], out=draws[i:i + 1])
    draws = draws.cpu()
    assert set(draws.tolist()) <= set(A), f"draws outside the allowed set: {sorted(set(draws.tolist()) - set(A))[:8]}"
    y = P.pick_values(bits, T)[A]
    p = np.exp(y - y.max())
    exp = torch.from_numpy(N * p / p.sum())
    counts = torch.tensor([(draws == n).sum().item() for n in A], dtype=torch.float64)
    mask = exp > 5
    chi2 = (((counts - exp) ** 2) / exp)[mask].sum().item()
    dof = int(mask.sum()) - 1
    print(f"chi2 {chi2:.1f} for {dof} dof over {int(mask.sum())} of 12 cells")
    assert dof >= 3 and chi2 < dof + 6 * (2 * dof) ** 0.5, f"chi2 {chi2:.1f} for {dof} dof"


# ----------------------------------------------------------------------------- 7. arguments
def test_argument_errors():
    ops = _ops()
    from unimedvl_amd import sampling
    from unimedvl_amd._lib import UmvError
    V = 40
    ref, host, dev = _automaton(V)
    logits = torch.zeros((1, V), dtype=BF16, device="cuda")
    state = torch.zeros(1, dtype=torch.int32, device="cuda")
    keys = torch.zeros((1, 3), dtype=torch.int64, device="cuda")
    stats = torch.zeros((1, 3, 2), dtype=torch.float32, device="cuda")
    table = sampling.to_tensor(sampling.pack([sampling.SamplingParams()]), "cuda")
    for kw in (dict(temperature=-0.5), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(lse_partial=stats),
               dict(argmax_partial=torch.zeros((1, 4), dtype=torch.int64, device="cuda")),               # not the tile count of V
               dict(argmax_partial=keys, sample_rows=table, temperature=0.7)):                           # a scalar temperature next to the table
        with pytest.raises(UmvError):
            ops.logit_constrain(logits, dev, state, **kw)
    with pytest.raises(UmvError):
        ops.logit_constrain(logits, dev, torch.zeros(2, dtype=torch.int32, device="cuda"))             # one word per row
    with pytest.raises(UmvError):
        ops.logit_constrain(logits, dev, state.to(torch.int64))
    with pytest.raises(UmvError):
        ops.logit_constrain(logits.float(), dev, state)
    with pytest.raises(UmvError):
        ops.logit_constrain(logits, host.to_device("cpu"), state)                                       # tables on the host
    with pytest.raises(UmvError):
        ops.constraint_advance(dev, state, torch.zeros(2, dtype=torch.int64, device="cuda"))
    with pytest.raises(UmvError):
        ops.constraint_advance(dev, state, torch.zeros(1, dtype=torch.int32, device="cuda"))

    class NoStates:                                       # the library's own check: an automaton without a state
        row_ptr, edge_token, edge_next = dev.row_ptr[:1], dev.edge_token[:0], dev.edge_next[:0]
        n_states, n_edges = 0, 0
    with pytest.raises(UmvError):
        ops.logit_constrain(logits, NoStates, state)
    with pytest.raises(UmvError):
        ops.constraint_advance(NoStates, state, torch.zeros(1, dtype=torch.int64, device="cuda"))
    ops.logit_constrain(logits, dev, state, argmax_partial=keys, lse_partial=stats)
    ops.constraint_advance(dev, state, torch.zeros(1, dtype=torch.int64, device="cuda"))
