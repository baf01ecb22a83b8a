"""umv_logit_penalty_bf16 (include/unimedvl_hip.h, "logit penalties and bias") at kernel level: the adjusted logits against the numpy
model of the definition (tests/penalty_ref.py), the recomputed tiles against the lm_head epilogue itself, the picks of the fused step
ends against the independent stand-alone entries on the patched logits, the recording, and batch independence.

Everything is asserted bit for bit, with two exceptions the header already bounds: a log-probability against umv_token_logprob_bf16 and
against the fp64 model is within the header's 1e-4.  The expected keys and statistics of a crafted row are the lm_head epilogue's own
for that row: x = e_0 and W[:, 0] = the model's adjusted row give exactly those logits, and whatever the epilogue then leaves in
argmax_partial / lse_partial is what the penalty kernel must have left."""
import functools

import numpy as np
import pytest
import torch

import penalty_ref as P

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
T = 0.7
SEED = 4321
K = 512
BOUND = 1e-4          # of a log-probability (include/unimedvl_hip.h, token log-probabilities)
MODES = [(0.0, False), (0.0, True), (T, False), (T, True)]        # (temperature: 0 = greedy, with lse_partial)
ON = dict(r=1.3, presence=0.5, frequency=0.25)


def _ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd import ops
    return ops


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _from_bits(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(BF16)


@functools.lru_cache(maxsize=None)
def _problem(M, V):
    """x [M, K] and the packed lm_head weight [V, K] on the device: logits ~ N(0, 3^2)"""
    ops = _ops()
    g = torch.Generator().manual_seed(100 * M + V)
    x = torch.randn(M, K, generator=g).to(BF16).cuda()
    w = (torch.randn(V, K, generator=g) * (3.0 / K ** 0.5)).to(BF16).cuda()
    return x, ops.PackedLinear.from_weight(w)


def _lm_head(x, lin, temp, lse, step=None):
    """the lm_head call: (logits, argmax_partial, lse_partial or None)"""
    ops = _ops()
    M, V = x.shape[0], lin.N
    nt = (V + 15) // 16
    out = torch.empty((M, (V + 7) // 8 * 8 + 8), dtype=BF16, device="cuda")[:, :V]      # a row stride beyond V (umv_argmax_bf16: ld % 8 == 0)
    keys = torch.zeros((M, nt), dtype=torch.int64, device="cuda")
    stats = torch.full((M, nt, 2), 55.0, dtype=torch.float32, device="cuda") if lse else None
    ops.gemm(x, lin, out=out, argmax_partial=keys, lse_partial=stats, sample=(temp, SEED, step) if temp > 0 else None)
    return out, keys, stats


def _row_lm_head(bits, temp, lse, step=None):
    """the epilogue's keys and statistics for ONE given row of logits: x = e_0, W[:, 0] = the row"""
    ops = _ops()
    V = len(bits)
    w = torch.zeros((V, 32), dtype=BF16)
    w[:, 0] = _from_bits(bits)
    x = torch.zeros((1, 32), dtype=BF16, device="cuda")
    x[0, 0] = 1.0
    out, keys, stats = _lm_head(x, ops.PackedLinear.from_weight(w.cuda()), temp, lse, step)
    got = _bits(out)[0]                  # (a -0 comes out of the accumulation as +0: the same key, the same y, the same exp)
    assert (P.same_bits(got, bits) | ((P.bf16_float(got) == 0) & (P.bf16_float(bits) == 0))).all(), "the one-hot GEMM must reproduce the row"
    return keys, stats


class State:
    """the device picture of a list of penalty_ref.History (one per row, same cap and n_static), with a guard word behind the list"""

    def __init__(self, hists):
        h0 = hists[0]
        self.M, self.cap, self.n_static = len(hists), h0.cap, h0.n_static
        self.count = torch.from_numpy(np.stack([h.count for h in hists]).view(np.int32)).cuda()
        buf = np.full(self.M * self.cap + 1, -77, dtype=np.int32)
        buf[:-1] = np.stack([h.list for h in hists]).reshape(-1)
        self.buf = torch.from_numpy(buf).cuda()
        self.list = self.buf[:-1].view(self.M, self.cap)
        self.len = torch.tensor([h.len for h in hists], dtype=torch.int32, device="cuda")
        self.bias = torch.from_numpy(np.stack([h.bias for h in hists])).cuda() if self.n_static else None

    def call(self, logits, ids, keys=None, stats=None, temp=0.0, step=None, r=1.0, presence=0.0, frequency=0.0):
        _ops().logit_penalty(logits, torch.as_tensor(ids, dtype=torch.int64).cuda(), self.count, self.list, self.len, self.n_static,
                             bias=self.bias, repetition_penalty=r, presence_penalty=presence, frequency_penalty=frequency,
                             temperature=temp, seed=SEED, step=step, argmax_partial=keys, lse_partial=stats)

    def check(self, hists):
        """count table, list, length and the guard word equal the model's"""
        assert np.array_equal(self.count.cpu().numpy().view(np.uint32), np.stack([h.count for h in hists])), "count table"
        assert np.array_equal(self.len.cpu().numpy(), np.array([h.len for h in hists], dtype=np.int32)), "list length"
        assert np.array_equal(self.list.cpu().numpy(), np.stack([h.list for h in hists])), "visit list"
        assert int(self.buf[-1]) == -77, "the word behind the list was written"


def _histories(M, V, n_gen=12, context=6, bias=True, extra=0):
    """one History per row with a context set, two biased columns (one of them in the context) and n_gen recorded tokens, some repeated"""
    rng = np.random.default_rng(7 * M + V)
    hists = []
    for m in range(M):
        ctx = rng.choice(V, size=context, replace=False).tolist()
        b = {int(ctx[0]): 1.5, int((ctx[1] + 1) % V): -2.25} if bias else None
        h = P.History(V, cap=context + 2 + n_gen + extra, context=ctx, bias=b, n_static=context + 2)
        h.record(0)                                   # the start token: the slot is no longer fresh
        toks = rng.choice(V, size=max(1, n_gen // 2), replace=False).tolist()
        for i in range(n_gen - 1):
            h.record(int(toks[i % len(toks)]) if i % 3 else int(ctx[2]))       # repeats, and a context column that is also generated
        hists.append(h)
    return hists


def _eq_stats(a, b):
    a, b = a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32)
    fa, fb = a.view(np.float32), b.view(np.float32)
    return ((a == b) | (np.isnan(fa) & np.isnan(fb))).all()


# ----------------------------------------------------------------------------- 1. neutral parameters change nothing
@pytest.mark.parametrize("M", [1, 8, 64])
@pytest.mark.parametrize("V", [40, 330, 4112])
def test_neutral_parameters_leave_every_bit(V, M):
    """r = 1, penalties 0, bias 0, with a list and a history: logits, keys and statistics after the kernel are the lm_head call's own -
    greedy keys, sampling keys (the noise stream) and the statistics' summation order, on every tile the list touches."""
    x, lin = _problem(M, V)
    step = torch.tensor([3], dtype=torch.int64, device="cuda")
    for temp, lse in MODES:
        out, keys, stats = _lm_head(x, lin, temp, lse, step)
        want = (out.clone(), keys.clone(), stats.clone() if lse else None)
        hists = _histories(M, V, bias=False)
        st = State(hists)
        ids = [(5 * m + 1) % V for m in range(M)]
        for h, t in zip(hists, ids):
            h.record(t)
        # poison the keys / statistics of the listed tiles: the kernel must write them back, not leave them
        at = [(m, n // 16) for m, h in enumerate(hists) for _, n in h.entries()]
        rows, tiles = (torch.tensor(v, device="cuda") for v in zip(*at))
        keys[rows, tiles] = 0
        if lse:
            stats[rows, tiles] = 55.0
        st.call(out, ids, keys, stats, temp, step)
        st.check(hists)
        assert torch.equal(out.view(torch.int16), want[0].view(torch.int16)), f"T={temp}: logits changed"
        assert torch.equal(keys, want[1]), f"T={temp} lse={lse}: the recomputed keys are not the epilogue's"
        if lse:
            assert _eq_stats(stats, want[2]), f"T={temp}: the recomputed statistics are not the epilogue's bits"


# ----------------------------------------------------------------------------- 2. the adjusted logits, crafted rows
def _crafted(V):
    """(row bits, History already recorded, the token fed now) cases on V columns"""
    rng = np.random.default_rng(V)
    base = P.bf16_bits((rng.standard_normal(V) * 3).astype(np.float32))
    cases = {}

    def row(**cols):
        b = base.copy()
        for n, v in cols.items():
            b[int(n[1:])] = P.bf16_bits(np.array([v], dtype=np.float32))[0]
        return b
    last = V - 1                                           # sits in the partial last tile (V = 40, 330)
    # counts 1 and 3, a column both in the context and generated, two listed columns in one tile (32, 35), one in the last tile
    h = P.History(V, cap=16, context=[3, 20], bias=None, n_static=4)
    for t in (0, 32, 35, 35, 35, 20, last):
        h.record(t)
    cases["counts"] = (row(c32=2.5, c35=-1.75, c20=0.8125, c3=-4.0), h, 32)
    # +0, -0, negative, -inf and NaN logits on seen columns
    h = P.History(V, cap=16, context=[1, 2], bias=None, n_static=2)
    for t in (0, 5, 6, 7, 8):
        h.record(t)
    cases["specials"] = (row(c1=0.0, c2=-0.0, c5=-0.0, c6=float("-inf"), c7=float("nan"), c8=-3.0, c9=0.0), h, 9)
    # a biased unseen column, and bias -inf on the raw argmax
    top = int(np.argmax(P.bf16_float(base)))
    h = P.History(V, cap=12, context=None, bias={(top + 7) % V: 2.75, top: float("-inf")}, n_static=3)
    h.record(0)
    cases["bias"] = (base.copy(), h, (top + 1) % V)
    # a tile fully banned: columns 16..31
    h = P.History(V, cap=20, context=None, bias={n: float("-inf") for n in range(16, 32)}, n_static=16)
    h.record(0)
    cases["banned tile"] = (base.copy(), h, 4)
    return cases


@pytest.mark.parametrize("r", [1.3, 0.8])
@pytest.mark.parametrize("V", [40, 330])
def test_adjusted_logits_match_the_model(V, r):
    par = dict(ON, r=r)
    step = torch.tensor([5], dtype=torch.int64, device="cuda")
    for name, (bits, hist, tok) in _crafted(V).items():
        for temp, lse in MODES:
            h = hist.copy()
            keys0, stats0 = _row_lm_head(bits, temp, lse, step)
            logits = _from_bits(bits).reshape(1, V).cuda()
            st = State([h])
            h.record(tok)
            want = P.adjust_row(bits, h, **par)
            st.call(logits, [tok], keys0, stats0, temp, step, **par)
            st.check([h])
            got = _bits(logits)[0]
            bad = np.flatnonzero(~P.same_bits(got, want))
            assert bad.size == 0, f"{name} T={temp}: columns {bad[:8]} got {got[bad[:8]]} want {want[bad[:8]]}"
            keys1, stats1 = _row_lm_head(want, temp, lse, step)
            assert torch.equal(keys0, keys1), f"{name} T={temp}: keys differ from the epilogue's on the adjusted row"
            if temp == 0:
                assert np.array_equal(keys0.cpu().numpy().view(np.uint64)[0], P.greedy_keys(want)), f"{name}: greedy keys against the model"
            if lse:
                assert _eq_stats(stats0, stats1), f"{name} T={temp}: statistics differ from the epilogue's on the adjusted row"
                if name == "banned tile":
                    assert stats0[0, 1].tolist() == [float("-inf"), 0.0]
        if name == "bias":
            top = int(np.argmax(P.bf16_float(bits)))
            assert P.bf16_float(want)[top] == float("-inf") and want[(top + 7) % V] != bits[(top + 7) % V]


def test_fresh_slot_changes_nothing_but_the_length_word():
    V = 330
    x, lin = _problem(8, V)
    out, keys, stats = _lm_head(x, lin, 0.0, True)
    want = (out.clone(), keys.clone(), stats.clone())
    hists = [P.History(V, cap=9, context=None, bias=None, n_static=0) for _ in range(8)]
    st = State(hists)
    for h in hists:
        h.record(11)
    st.call(out, [11] * 8, keys, stats, **ON)
    st.check(hists)
    assert (st.len == 0).all() and (st.count == 0).all()
    assert torch.equal(out.view(torch.int16), want[0].view(torch.int16)) and torch.equal(keys, want[1]) and _eq_stats(stats, want[2])


# ----------------------------------------------------------------------------- 3. picks against the independent entries
def _step_bufs(B, max_len, s):
    dev = "cuda"
    return dict(slot=torch.zeros(B, dtype=torch.int32, device=dev), pos=torch.zeros(B, dtype=torch.int32, device=dev),
                kvl=torch.ones(B, dtype=torch.int32, device=dev), ids=torch.full((B,), -5, dtype=torch.int64, device=dev),
                in_ids=torch.zeros((max_len, B), dtype=torch.int64, device=dev), pred=torch.zeros((max_len, B), dtype=torch.int64, device=dev),
                step=torch.full((B,), s, dtype=torch.int64, device=dev), lp=torch.zeros((max_len, B), dtype=torch.float32, device=dev),
                cut=torch.zeros((max_len, B), dtype=torch.float32, device=dev), kept=torch.zeros((max_len, B), dtype=torch.int32, device=dev))


def _penalised(M, V, temp, lse, s=2):
    """lm_head call, then the kernel with penalties on and the raw argmax banned: (patched logits, keys, stats, step buffers)"""
    x, lin = _problem(M, V)
    b = _step_bufs(M, 4, s)
    out, keys, stats = _lm_head(x, lin, temp, lse, b["step"])
    raw_top = out.float().argmax(-1).tolist()
    rng = np.random.default_rng(V + M)
    hists = []
    for m in range(M):
        ctx = rng.choice(V, size=5, replace=False).tolist()
        up = next(n for n in range(ctx[0] + 3, ctx[0] + 5) if n % V != raw_top[m]) % V
        h = P.History(V, cap=24, context=ctx, bias={raw_top[m]: float("-inf"), up: 1.25}, n_static=7)
        for t in [0] + rng.choice(V, size=8).tolist() + [ctx[1]]:
            h.record(int(t))
        hists.append(h)
    st = State(hists)
    ids = rng.choice(V, size=M).tolist()
    raw = _bits(out)
    st.call(out, ids, keys, stats, temp, b["step"], **ON)
    for m, (h, t) in enumerate(zip(hists, ids)):
        h.record(int(t))
        assert P.same_bits(_bits(out[m]), P.adjust_row(raw[m], h, **ON)).all(), f"row {m}: adjusted logits against the model"
    return out, keys, stats, b, raw_top


@pytest.mark.parametrize("M", [1, 8, 64])
@pytest.mark.parametrize("V", [40, 330, 4112])
def test_fused_picks_equal_the_stand_alone_entries_on_the_patched_logits(V, M):
    ops = _ops()
    s = 2
    # greedy: umv_decode_step_end_argmax against umv_argmax_bf16
    out, keys, _, b, raw_top = _penalised(M, V, 0.0, False, s)
    ops.decode_step_end_argmax(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"])
    assert torch.equal(b["ids"], ops.argmax(out)), "greedy"
    assert all(int(i) != t for i, t in zip(b["ids"].tolist(), raw_top)), "the banned raw argmax was picked"
    # greedy log-probability: umv_decode_step_end_logprob against umv_token_logprob_bf16 and the fp64 model
    out, keys, stats, b, _ = _penalised(M, V, 0.0, True, s)
    ops.decode_step_end_logprob(b["slot"], b["pos"], b["kvl"], keys, stats, b["ids"], b["in_ids"], b["pred"], b["step"], out, b["lp"], 0.0)
    alone = ops.token_logprob(out, b["ids"], 0.0)
    bits = _bits(out)
    model = torch.tensor([P.logprob(bits[m], int(b["ids"][m])) for m in range(M)])
    print(f"V={V} M={M}: logprob vs stand-alone {float((b['lp'][s] - alone).abs().max()):.3g}, vs fp64 "
          f"{float((b['lp'][s].cpu().double() - model).abs().max()):.3g}")
    assert float((b["lp"][s] - alone).abs().max()) <= BOUND and float((b["lp"][s].cpu().double() - model).abs().max()) <= BOUND
    # sampling: the step end on the sampling keys against umv_sample_bf16 with the same (seed, step)
    out, keys, _, b, _ = _penalised(M, V, T, False, s)
    st = b["step"][:1].clone()
    ops.decode_step_end_argmax(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"])
    assert torch.equal(b["ids"], ops.sample(out, T, SEED, step=st)), "sampling"
    # truncated sampling (with log-probabilities): umv_decode_step_end_truncated against umv_sample_truncated_bf16
    out, keys, stats, b, _ = _penalised(M, V, T, True, s)
    flt = dict(top_k=5, top_p=0.8)
    cut = torch.zeros(M, dtype=torch.float32, device="cuda")
    kept = torch.zeros(M, dtype=torch.int32, device="cuda")
    alone = ops.sample_truncated(out, T, SEED, step=b["step"][:1].clone(), cut_y=cut, n_kept=kept, **flt)
    ops.decode_step_end_truncated(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"], out, T, SEED,
                                  lse_partial=stats, logprobs=b["lp"], cut_y=b["cut"], n_kept=b["kept"], **flt)
    assert torch.equal(b["ids"], alone) and torch.equal(b["cut"][s], cut) and torch.equal(b["kept"][s], kept), "truncated"
    lp = ops.token_logprob(out, b["ids"], T)
    assert float((b["lp"][s] - lp).abs().max()) <= BOUND, "truncated step end: log-probability of the adjusted, untruncated softmax"


# ----------------------------------------------------------------------------- 4. recording
def test_recording_follows_the_model_and_stops_at_cap():
    """k calls with known ids, one token recurring: count table, list (distinct) and length equal the model's after every call; the
    history is chosen to fill the list exactly to cap, then two more new tokens find no room: counted, not listed, nothing written at
    or beyond cap (the guard word behind the one-row list; row 1's first static entry behind row 0's list)."""
    V, cap = 330, 9
    for M in (1, 2):
        hists = [P.History(V, cap=cap, context=[4, 5], bias={6: 1.0}, n_static=4) for _ in range(M)]
        st = State(hists)
        logits = torch.zeros((M, V), dtype=BF16, device="cuda")
        seq = [17, 100, 100, 5, 329, 100, 6, 200, 201, 17, 250, 251, 100]      # 17 is the start token; 5 new columns fill 4 + 5 = cap
        for i, t in enumerate(seq):
            ids = [t if m == 0 else (t + 1) % V for m in range(M)]
            for h, tok in zip(hists, ids):
                h.record(tok)
            st.call(logits, ids, **ON)
            st.check(hists)
            lst = st.list[0, :int(st.len[0])].tolist()
            assert len(set(lst) - {-1}) == len([c for c in lst if c != -1]), "the list is distinct"
        assert int(st.len[0]) == cap and hists[0].count[250] & P.COUNT_MASK == 1 and not hists[0].count[250] & P.LISTED


def test_unfused_use_patches_without_partials():
    V, M = 330, 8
    x, lin = _problem(M, V)
    out, _, _ = _lm_head(x, lin, 0.0, False)
    raw = _bits(out)
    hists = _histories(M, V)
    st = State(hists)
    ids = [(3 * m + 2) % V for m in range(M)]
    for h, t in zip(hists, ids):
        h.record(t)
    st.call(out, ids, **ON)
    st.check(hists)
    for m in range(M):
        assert P.same_bits(_bits(out[m]), P.adjust_row(raw[m], hists[m], **ON)).all()


# ----------------------------------------------------------------------------- 5. batch independence, arguments
@pytest.mark.parametrize("V", [330, 4112])
def test_a_row_does_not_depend_on_its_batch(V):
    """row i of an M = 64 call equals the same row run alone at M = 1, bit for bit: logits, keys, statistics.  (The sampling key of a
    row names the row, so the lone run is the greedy one plus the sampling one for row 0.)"""
    M = 64
    x, lin = _problem(M, V)
    for temp in (0.0, T):
        out, keys, stats = _lm_head(x, lin, temp, True)
        hists = _histories(M, V)
        ids = [(7 * m + 3) % V for m in range(M)]
        many = State(hists)
        raw = out.clone()
        many.call(out, ids, keys, stats, temp, **ON)
        for i in ((0, 17, 63) if temp == 0 else (0,)):
            o1, k1, s1 = _lm_head(x[i:i + 1].contiguous(), lin, temp, True)
            assert torch.equal(o1.view(torch.int16), raw[i:i + 1].view(torch.int16))
            State([hists[i]]).call(o1, [ids[i]], k1, s1, temp, **ON)
            assert torch.equal(o1.view(torch.int16), out[i:i + 1].view(torch.int16)) and torch.equal(k1, keys[i:i + 1]) \
                and _eq_stats(s1, stats[i:i + 1]), f"row {i} T={temp}"


def test_argument_errors():
    ops = _ops()
    from unimedvl_amd._lib import UmvError
    V = 40
    st = State([P.History(V, cap=6, context=[1], bias=None, n_static=1)])
    logits = torch.zeros((1, V), dtype=BF16, device="cuda")
    keys = torch.zeros((1, 3), dtype=torch.int64, device="cuda")
    stats = torch.zeros((1, 3, 2), dtype=torch.float32, device="cuda")
    for kw in (dict(r=0.0), dict(r=-1.0), dict(r=float("inf")), dict(r=float("nan")), dict(presence=float("inf")),
               dict(frequency=float("nan")), dict(temp=-0.5), dict(stats=stats)):
        with pytest.raises(UmvError):
            st.call(logits, [0], **kw)
    with pytest.raises(UmvError):
        st.call(logits, [0], keys=torch.zeros((1, 4), dtype=torch.int64, device="cuda"))       # not the tile count of V
    with pytest.raises(UmvError):                                                             # cap below the static length
        ops.logit_penalty(logits, torch.zeros(1, dtype=torch.int64, device="cuda"), st.count, st.list, st.len, 7)
    st.call(logits, [0], keys, stats)
