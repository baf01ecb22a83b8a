"""Per-row sampling parameters (include/unimedvl_hip.h, umv_row_sampling) at kernel level.  The yardstick is the scalar entries: every
per-row definition is the scalar definition with the row's own values, so a table whose rows hold the values of a scalar call - with
stream = row index, draw = step, the same seed - must leave that call's bits everywhere: the logits, the keys and (max, sum exp) after
the lm_head call and after the penalty launch, and everything the step end writes.  A mixed table equals, row by row, the scalar call in
which all rows have that row's parameters.  No tolerance anywhere; the distribution test uses the project's chi-square bound."""
import functools

import numpy as np
import pytest
import torch

import penalty_ref as P
import truncation_ref as R
from test_logit_penalty_gpu import State

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
T = 0.7
SEED = 4321
S = 3                 # the step of the scalar calls = the draw of the table rows
MAX_LEN = 6
NEUTRAL = dict(temp=0.0, top_k=0, top_p=1.0, min_p=0.0, r=1.0, presence=0.0, frequency=0.0)
PEN = dict(r=1.3, presence=0.5, frequency=0.25)
SAMPLERS = {"greedy": {}, "T": dict(temp=T), "top_k": dict(temp=T, top_k=5), "top_p": dict(temp=T, top_p=0.8),
            "min_p": dict(temp=T, min_p=0.1), "all": dict(temp=T, top_k=12, top_p=0.9, min_p=0.02)}
# the five sets of the mixed table: greedy, plain sampling, truncated, penalised (greedy), truncated + penalised
MIXED = [{}, dict(temp=T), dict(temp=T, top_k=5, top_p=0.8), dict(PEN), dict(temp=1.1, top_p=0.6, **PEN)]


def _ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd import ops
    return ops


def _par(**kw):
    return dict(NEUTRAL, **kw)


def _table(pars, streams, draws, seed=SEED):
    """the device table of a list of parameter dicts, packed field by field (not through SamplingParams: the kernels' contract)"""
    from unimedvl_amd import sampling
    t = np.zeros(len(pars), dtype=sampling.ROW_DTYPE)
    for i, p in enumerate(pars):
        p = _par(**p)
        t[i] = (seed, draws[i], streams[i], p["temp"], p["top_k"], p["top_p"], p["min_p"], p["r"], p["presence"], p["frequency"])
    return sampling.to_tensor(t, "cuda")


@functools.lru_cache(maxsize=None)
def _problem(M, V, image):
    """x = e_0 in every row, so every row's logits are W[:, 0] ~ N(0, 2^2); the lm_head image: bf16, the forced 13-bit one, or e4m3"""
    ops = _ops()
    K = 64 if image == "z13" else 32              # the 13-bit image codes 64-k units
    g = torch.Generator().manual_seed(81 + V)
    w = torch.zeros((V, K))
    w[:, 0] = torch.randn(V, generator=g) * 2
    w = w.to(BF16).cuda()
    x = torch.zeros((M, K), dtype=BF16, device="cuda")
    x[:, 0] = 1.0
    if image == "e4m3":
        return x, ops.PackedLinear.from_weight_fp8(w), None
    lin = ops.PackedLinear.from_weight(w)
    if image == "z13":
        lin.build_z13()
        return x, lin, True
    return x, lin, False


def _step_bufs(B, s):
    dev = "cuda"
    return dict(slot=torch.arange(10, 10 + B, dtype=torch.int32, device=dev), pos=torch.arange(20, 20 + B, dtype=torch.int32, device=dev),
                kvl=torch.arange(11, 11 + B, dtype=torch.int32, device=dev), ids=torch.full((B,), -5, dtype=torch.int64, device=dev),
                in_ids=torch.full((MAX_LEN, B), -7, dtype=torch.int64, device=dev),
                pred=torch.full((MAX_LEN, B), -9, dtype=torch.int64, device=dev),
                step=torch.full((B,), s, dtype=torch.int64, device=dev),
                lp=torch.full((MAX_LEN, B), 99.0, dtype=torch.float32, device=dev),
                cut=torch.full((MAX_LEN, B), 77.0, dtype=torch.float32, device=dev),
                kept=torch.full((MAX_LEN, B), -3, dtype=torch.int32, device=dev))


def _histories(M, V):
    """one History per row: a context set, a few recorded tokens (some repeated), no bias"""
    rng = np.random.default_rng(7 * M + V)
    hists = []
    for m in range(M):
        ctx = rng.choice(V, size=4, replace=False).tolist()
        h = P.History(V, cap=4 + 10, context=ctx, bias=None, n_static=4)
        h.record(0)
        toks = rng.choice(V, size=4, replace=False).tolist()
        for i in range(7):
            h.record(int(toks[i % 4]) if i % 3 else int(ctx[1]))
        hists.append(h)
    return hists


def _bits(t):
    if t.dtype == BF16:
        return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
    if t.dtype == torch.float32:
        return t.detach().cpu().contiguous().numpy().view(np.uint32)
    return t.detach().cpu().contiguous().numpy()


def _run(M, V, image, s=S, par=None, rows=None, pen=False, lse=False):
    """One step's tail: lm_head call, optionally the penalty launch, the step end.  par: the scalar call (all rows alike, the scalar
    entries); rows: the per-row table (the new ones).  Returns every buffer the three launches write, as bits."""
    ops = _ops()
    x, lin, z13 = _problem(M, V, image)
    b = _step_bufs(M, s)
    nt = (V + 15) // 16
    out = torch.empty((M, V), dtype=BF16, device="cuda")
    keys = torch.zeros((M, nt), dtype=torch.int64, device="cuda")
    stats = torch.full((M, nt, 2), 55.0, dtype=torch.float32, device="cuda") if lse else None
    res = {}
    table0 = None if rows is None else rows.clone()
    if rows is None:
        p = _par(**par)
        ops.gemm(x, lin, out=out, argmax_partial=keys, lse_partial=stats, sample=(p["temp"], SEED, b["step"]) if p["temp"] > 0 else None,
                 z13=z13)
    else:
        ops.gemm(x, lin, out=out, argmax_partial=keys, lse_partial=stats, sample_rows=rows, z13=z13)
    res.update(logits0=_bits(out), keys0=_bits(keys), stats0=None if stats is None else _bits(stats))
    if pen:
        hists = _histories(M, V)
        st = State(hists)
        fed = torch.tensor([(5 * m + 1) % V for m in range(M)], dtype=torch.int64, device="cuda")
        if rows is None:
            ops.logit_penalty(out, fed, st.count, st.list, st.len, st.n_static, repetition_penalty=p["r"], presence_penalty=p["presence"],
                              frequency_penalty=p["frequency"], temperature=p["temp"], seed=SEED, step=b["step"], argmax_partial=keys,
                              lse_partial=stats)
        else:
            ops.logit_penalty(out, fed, st.count, st.list, st.len, st.n_static, argmax_partial=keys, lse_partial=stats, sample_rows=rows)
        res.update(logits1=_bits(out), keys1=_bits(keys), stats1=None if stats is None else _bits(stats), count=_bits(st.count),
                   vlist=_bits(st.list), vlen=_bits(st.len))
    if rows is not None:
        assert torch.equal(rows, table0), "the GEMM and the penalty launch only read the table"
        ops.decode_step_end_rows(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"], out, rows,
                                 lse_partial=stats, logprobs=b["lp"] if lse else None, cut_y=b["cut"], n_kept=b["kept"])
        want = table0.clone()
        want[:, 1] += 1
        assert torch.equal(rows, want), "the step end adds 1 to every row's draw and writes no other word of the table"
    elif p["temp"] > 0 and (p["top_k"] > 0 or p["top_p"] < 1.0 or p["min_p"] > 0.0):
        ops.decode_step_end_truncated(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"], out, p["temp"], SEED,
                                      top_k=p["top_k"], top_p=p["top_p"], min_p=p["min_p"], lse_partial=stats,
                                      logprobs=b["lp"] if lse else None, cut_y=b["cut"], n_kept=b["kept"])
    else:                                         # the key maximum: cut_y = -inf, n_kept = V by the per-row entry's definition
        if lse:
            ops.decode_step_end_logprob(b["slot"], b["pos"], b["kvl"], keys, stats, b["ids"], b["in_ids"], b["pred"], b["step"], out, b["lp"],
                                        p["temp"])
        else:
            ops.decode_step_end_argmax(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"])
        b["cut"][s] = float("-inf")
        b["kept"][s] = V
    res.update({k: _bits(v) for k, v in b.items()})
    res["_keys"], res["_out"] = keys, out
    return res


def _same(a, b, what, rows=None):
    """every buffer of two runs equal bit for bit (rows: only these rows of the per-row buffers)"""
    for k in a:
        if k.startswith("_") or a[k] is None:
            continue
        u, v = a[k], b[k]
        if rows is not None:
            ax = 1 if k in ("in_ids", "pred", "lp", "cut", "kept") else 0
            u, v = np.take(u, rows, axis=ax), np.take(v, rows, axis=ax)
        assert np.array_equal(u, v), f"{what}: {k} differs"


# ----------------------------------------------------------------------------- 1. a uniform table equals the scalar call
@pytest.mark.parametrize("image", ["bf16", "z13", "e4m3"])
@pytest.mark.parametrize("M", [1, 8, 64])
@pytest.mark.parametrize("V", [40, 330, 4112])
def test_uniform_table_equals_the_scalar_call(V, M, image):
    for name, smp in SAMPLERS.items():
        for pen in (False, True):
            for lse in (False, True):
                par = dict(smp, **(PEN if pen else {}))
                want = _run(M, V, image, par=par, pen=pen, lse=lse)
                rows = _table([par] * M, streams=list(range(M)), draws=[S] * M)
                got = _run(M, V, image, rows=rows, pen=pen, lse=lse)
                _same(want, got, f"{name} pen={pen} lse={lse}")
                assert (got["step"] == S + 1).all() and (got["slot"] == np.arange(11, 11 + M)).all()


# ----------------------------------------------------------------------------- 2. a mixed table equals the scalar call row by row
def _key_ids(keys):
    k = keys.cpu().numpy().view(np.uint64).max(axis=1)
    return (np.uint64(0xFFFFFFFF) - (k & np.uint64(0xFFFFFFFF))).astype(np.int64)


@pytest.mark.parametrize("M", [8, 64])
@pytest.mark.parametrize("V", [40, 330, 4112])
def test_mixed_table_equals_the_scalar_call_row_by_row(V, M):
    """row m holds set m % 5, so greedy and sampled rows share every 16-row fragment; log-probabilities on for the whole launch"""
    pars = [MIXED[m % 5] for m in range(M)]
    rows = _table(pars, streams=list(range(M)), draws=[S] * M)
    got = _run(M, V, "bf16", rows=rows, pen=True, lse=True)
    for j, par in enumerate(MIXED):
        mine = [m for m in range(M) if m % 5 == j]
        pen = "r" in par
        want = _run(M, V, "bf16", par=par, pen=pen, lse=True)
        if not pen:                # a neutral row of the penalty launch keeps every bit the lm_head call left; its history is recorded
            want.update(logits1=want["logits0"], keys1=want["keys0"], stats1=want["stats0"])
            want.update({k: got[k] for k in ("count", "vlist", "vlen")})
        _same(want, got, f"set {j}", rows=mine)
    hists = _histories(M, V)
    for m, h in enumerate(hists):
        h.record((5 * m + 1) % V)
    assert np.array_equal(got["count"].view(np.uint32), np.stack([h.count for h in hists])), "every row's history is recorded"
    # the three branches of the step end in this one launch: the key maximum, the fused pick kept, the re-draw over the kept set
    fused = _key_ids(got["_keys"])
    logits = got["_out"].cpu()
    n_max = n_fast = n_slow = 0
    for m, par in enumerate(pars):
        p = _par(**par)
        if not (p["temp"] > 0 and (p["top_k"] > 0 or p["top_p"] < 1.0)):
            n_max += 1
            assert got["ids"][m] == fused[m] and got["kept"][S, m] == V and got["cut"].view(np.float32)[S, m] == float("-inf")
            continue
        y = R.pick_value(logits[m], p["temp"])
        i, cut_ref, n_ref = R.cutoff(R.classes(y), top_k=p["top_k"], top_p=p["top_p"], min_p=p["min_p"])
        assert got["cut"].view(np.float32)[S, m] == np.float32(cut_ref) and got["kept"][S, m] == n_ref, f"row {m}: cutoff"
        assert float(y[got["ids"][m]]) >= cut_ref, f"row {m}: the pick lies outside the kept set"
        if float(y[fused[m]]) >= cut_ref:
            n_fast += 1
            assert got["ids"][m] == fused[m]
        else:
            n_slow += 1
    print(f"V={V} M={M}: key maximum {n_max}, fused pick kept {n_fast}, re-drawn {n_slow}")
    if M == 64:
        assert n_max > 0 and n_fast > 0 and n_slow > 0, f"one launch must take all three branches ({n_max}, {n_fast}, {n_slow})"


# ----------------------------------------------------------------------------- 3. slot independence
@pytest.mark.parametrize("V", [330, 4112])
def test_a_request_does_not_depend_on_its_row(V):
    """the same (seed, stream, draw), parameters and logits at another row index: the same keys, statistics, pick, cutoff and
    log-probability - rows m and m + 4 of one call, and the same request alone at row 0 of a one-row call"""
    M = 8
    sets = [MIXED[1], MIXED[2], SAMPLERS["all"], MIXED[0]]
    pars = [sets[m % 4] for m in range(M)]
    rows = _table(pars, streams=[5] * M, draws=[9] * M, seed=99)
    got = _run(M, V, "bf16", rows=rows, lse=True)
    for m in range(4):
        for k in ("keys0", "stats0", "ids"):
            assert np.array_equal(got[k][m], got[k][m + 4]), f"{k}: rows {m} and {m + 4}"
        for k in ("pred", "in_ids", "lp", "cut", "kept"):
            assert np.array_equal(got[k][:, m], got[k][:, m + 4]), f"{k}: rows {m} and {m + 4}"
        alone = _run(1, V, "bf16", rows=_table([pars[m]], streams=[5], draws=[9], seed=99), lse=True)
        for k in ("keys0", "stats0", "ids"):
            assert np.array_equal(got[k][m], alone[k][0]), f"{k}: row {m} against the one-row call"
        for k in ("pred", "lp", "cut", "kept"):
            assert np.array_equal(got[k][S, m], alone[k][S, 0]), f"{k}: row {m} against the one-row call"
    other = _run(M, V, "bf16", rows=_table(pars, streams=[5] * M, draws=[10] * M, seed=99), lse=True)
    assert not np.array_equal(got["keys0"][:3], other["keys0"][:3]), "another draw counter names other noise"
    assert np.array_equal(got["keys0"][3], other["keys0"][3]), "a greedy row has no noise"


# ----------------------------------------------------------------------------- 4. the distribution
def test_frequencies_follow_each_rows_truncated_softmax():
    """ONE step-end launch over stored logits, 4 x 16 384 rows alternating between two temperatures and two filters.  The keys are
    empty (no untruncated pick to keep), so every row draws its Gumbel maximum over its kept set with its own (seed, stream, draw)."""
    ops = _ops()
    V, per = 40, 16384
    classes = [dict(temp=0.7, top_p=0.8), dict(temp=1.3, top_k=7), dict(temp=0.7, top_k=7), dict(temp=1.3, top_p=0.8)]
    B = per * len(classes)
    g = torch.Generator().manual_seed(81)
    one = (torch.randn(V, generator=g) * 0.7).to(BF16)
    logits = one.expand(B, V).contiguous().cuda()
    pars = [classes[m % 4] for m in range(B)]
    rows = _table(pars, streams=[m // 4 for m in range(B)], draws=[m % 7 for m in range(B)], seed=2024)
    b = _step_bufs(B, 0)
    keys = torch.zeros((B, 3), dtype=torch.int64, device="cuda")
    ops.decode_step_end_rows(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"], logits, rows,
                             cut_y=b["cut"], n_kept=b["kept"])
    ids, cut, kept = b["ids"].cpu(), b["cut"][0].cpu(), b["kept"][0].cpu()
    for j, c in enumerate(classes):
        y = R.pick_value(one, c["temp"])
        row = R.classes(y)
        i, cut_ref, n_ref = R.cutoff(row, top_k=c.get("top_k", 0), top_p=c.get("top_p", 1.0))
        p = R.truncated_probs(row, y, i)
        assert 3 <= n_ref < V
        assert (cut[j::4] == cut_ref).all() and (kept[j::4] == n_ref).all(), f"class {j}: cutoff"
        counts = torch.bincount(ids[j::4], minlength=V).double()
        assert counts.sum() == per and counts[p == 0].sum() == 0, f"class {j}: a draw outside the kept set"
        exp = p * per
        mask = exp > 5
        chi2 = (((counts - exp) ** 2) / exp)[mask].sum().item()
        dof = int(mask.sum()) - 1
        print(f"class {j} {c}: chi2 {chi2:.1f} for {dof} dof, {n_ref} columns kept")
        assert chi2 < dof + 6 * (2 * dof) ** 0.5, f"class {j}: chi2 {chi2:.1f} for {dof} dof"


# ----------------------------------------------------------------------------- 5. refusals
def test_refusals_and_a_greedy_row_with_filters():
    ops = _ops()
    from unimedvl_amd import _lib
    from unimedvl_amd._lib import UmvError
    V, M = 40, 8
    x, lin, _ = _problem(M, V, "bf16")
    rows = _table([{}] * M, list(range(M)), [0] * M)
    out = torch.empty((M, V), dtype=BF16, device="cuda")
    keys = torch.zeros((M, 3), dtype=torch.int64, device="cuda")
    step = torch.zeros(M, dtype=torch.int64, device="cuda")
    with pytest.raises(UmvError):                                   # without argmax_partial
        ops.gemm(x, lin, out=out, sample_rows=rows)
    with pytest.raises(UmvError):                                   # next to a scalar sampling temperature
        ops.gemm(x, lin, out=out, argmax_partial=keys, sample=(T, SEED, step), sample_rows=rows)
    x65 = torch.zeros((65, 32), dtype=BF16, device="cuda")
    with pytest.raises(UmvError):                                   # above 64 rows
        ops.gemm(x65, lin, out=torch.empty((65, V), dtype=BF16, device="cuda"),
                 argmax_partial=torch.zeros((65, 3), dtype=torch.int64, device="cuda"), sample_rows=_table([{}] * 65, [0] * 65, [0] * 65))
    ops.gemm(x, lin, out=out, argmax_partial=keys, sample_rows=rows)
    st = State([P.History(V, cap=6, context=[1], bias=None, n_static=1) for _ in range(M)])
    fed = torch.zeros(M, dtype=torch.int64, device="cuda")
    for kw in (dict(repetition_penalty=1.2), dict(presence_penalty=0.5), dict(frequency_penalty=0.1), dict(temperature=T)):
        with pytest.raises(UmvError):                               # non-neutral scalars next to the table
            ops.logit_penalty(out, fed, st.count, st.list, st.len, st.n_static, argmax_partial=keys, sample_rows=rows, **kw)
    b = _step_bufs(M, 0)
    with pytest.raises(UmvError):                                   # no table
        ops.decode_step_end_rows(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"], out, None)
    with pytest.raises(UmvError):                                   # log-probabilities without the statistics
        ops.decode_step_end_rows(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"], out, rows, logprobs=b["lp"])
    # B == 0 is fine and writes nothing
    before = rows.clone()
    p = lambda t: t.data_ptr()
    rc = _lib.load().umv_decode_step_end_rows(p(b["slot"]), p(b["pos"]), p(b["kvl"]), p(keys), None, 3, p(b["ids"]), p(b["in_ids"]), p(b["pred"]),
                                              p(b["step"]), p(out), out.stride(0), V, None, None, 0, MAX_LEN, p(rows), None, None, None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(rows, before) and (b["ids"] == -5).all()
    # a greedy row with filters set is greedy
    want = _run(M, V, "bf16", par={}, lse=True)
    got = _run(M, V, "bf16", rows=_table([dict(temp=0.0, top_k=3, top_p=0.5, min_p=0.3), dict(temp=-1.0, top_k=2),
                                          dict(temp=float("nan"), top_p=0.1)] * 2 + [{}] * 2, list(range(M)), [S] * M), lse=True)
    _same(want, got, "greedy rows with filters")
