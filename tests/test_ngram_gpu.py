"""umv_logit_ngram_ban_bf16 (include/unimedvl_hip.h, "no-repeat n-grams") at kernel level, bit for bit against the plain-Python
definition (tests/ngram_ref.py): the banned logits, the history record, the recomputed tiles against the lm_head epilogue itself, the
words nothing may touch, the picks of the fused step ends against the stand-alone entries, batch independence and the argument checks.

The expected keys and statistics of a row are the lm_head epilogue's own for the reference's banned row: x = e_0 in every row of the
call and W[:, 0] = that row give exactly those logits in every row of the GEMM - row m of it with row m's sampling key - and whatever
the epilogue leaves in argmax_partial[m] / lse_partial[m] is what the kernel must have left on the tiles it touched (the device of
tests/test_logit_penalty_gpu.py, for a row that sits at index m).  The only tolerance is the header's 1e-4 on a log-probability."""
import functools

import numpy as np
import pytest
import torch

import ngram_ref as R
import penalty_ref as P

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
T = 0.7
SEED = 4321
BOUND = 1e-4          # of a log-probability (include/unimedvl_hip.h, token log-probabilities)
MODES = [(0.0, False), (0.0, True), (T, False), (T, True)]        # (temperature: 0 = greedy, with lse_partial)
HIST_LD = 1002
NAN, NINF = 0x7FC0, 0xFF80
KEY_FILL, STAT_FILL, GUARD = 0x0123456789ABCDEF, 55.0, -77
SIZES = (1, 2, 3, 4, 16)


def _ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd import ops
    return ops


def _from_bits(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(BF16)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _same_words(a, b):
    """fp32 words equal bit for bit, a NaN equal to any NaN (a row that holds a NaN logit)"""
    fa, fb = a.view(np.float32), b.view(np.float32)
    return ((a == b) | (np.isnan(fa) & np.isnan(fb))).all()


def _letters(V):
    """four columns: two in one tile, one in the (partial, for V = 40 / 330) last tile"""
    return [3, 17, 18, V - 1]


@functools.lru_cache(maxsize=None)
def _cases(V):
    """[(name, history before the call, fed token, n)]: per size the lengths {0, n-2, n-1, n, 255, 256, 257, 1000, hist_ld - 1,
    hist_ld}, on periodic sequences over 2-4 letters and random ones over 4; then the rows with separators and out-of-range entries"""
    a, b, c, d = _letters(V)
    rng = np.random.default_rng(V)
    out = []
    for n in SIZES:
        for L0 in sorted({v for v in (0, n - 2, n - 1, n, 255, 256, 257, 1000, HIST_LD - 1, HIST_LD) if v >= 0}):
            kinds = [("periodic3", [(a, b, c)[i % 3] for i in range(L0 + 1)])]
            if L0 >= 255:
                kinds += [("periodic2", [(d, b)[i % 2] for i in range(L0 + 1)]), ("periodic4", [(a, b, c, d)[i % 4] for i in range(L0 + 1)]),
                          ("random4", [(a, b, c, d)[i] for i in rng.integers(0, 4, L0 + 1)])]
            for kind, seq in kinds:
                out.append((f"n={n} len={L0} {kind}", seq[:L0], seq[L0], n))
    big = V + 7
    out += [
        ("separator between the n-grams", [a, b, c, -1, a], b, 3),              # bans c
        ("separator in the suffix", [a, -1, c, a], -1, 3),                      # (a, -1) equals (a, -1) as integers: still no match
        ("out-of-range id in the suffix", [a, big, c, a], big, 3),
        ("follower out of range", [a, b, big, a], b, 3),
        ("follower a separator", [a, b, -1, a], b, 3),
        ("separator in the prefix only", [-1, b, c, a, b, d, a], b, 3),         # bans d; (-1, b) is no match
        ("fed id beyond int32", [a, b, a], (1 << 31) + a, 2),                   # recorded as -1
        ("fed id negative", [a, b, a], -(1 << 40), 2),
        ("n=1 with separators", [a, -1, big, b, a], c, 1),                      # bans a, b, c
        ("n=2 overlap", [a], a, 2),                                             # a a: bans a
        ("n=2 two followers one tile", [a, b, a, c, a, b], a, 2),               # bans b (17) and c (18)
        ("off", [a, b, a], b, 2),
        ("off full", [a, b, a], b, 2),
    ]
    return out


def _case_history(case):
    name, pre, tok, n = case
    h = R.History(HIST_LD, pre)
    if name == "off":
        h.len = -1
    elif name == "off full":
        h.len = R.FULL
    return h


def _base_row(V, r):
    """a row of logits ~ N(0, 3^2) with, in turn, a NaN and a -inf on a letter column"""
    rng = np.random.default_rng(1000 * V + r)
    bits = P.bf16_bits((rng.standard_normal(V) * 3).astype(np.float32))
    a, b, c, d = _letters(V)
    if r % 3 == 1:
        bits[a] = bits[d] = NAN
    elif r % 3 == 2:
        bits[b] = bits[c] = NINF
    return bits


def _guarded(data, dtype, guard):
    """a device tensor of `data` with one guard word behind it: (the view, the whole buffer)"""
    flat = np.ascontiguousarray(data).reshape(-1)
    buf = torch.empty(flat.size + 1, dtype=dtype, device="cuda")
    buf[:-1] = _from_bits(flat) if dtype == BF16 else torch.from_numpy(flat)
    buf[-1] = guard
    return buf[:-1].view(*data.shape), buf


def _table(M, temp):
    """a per-row table whose rows all sample at `temp` (0: greedy), each with a seed, draw and stream of its own"""
    from unimedvl_amd import sampling
    ps = [sampling.SamplingParams(do_sample=temp > 0, temperature=temp if temp > 0 else 1.0, seed=900 + 7 * m) for m in range(M)]
    return sampling.to_tensor(sampling.pack(ps, streams=[(3 * m + 1) % 11 for m in range(M)], draws=[m % 5 for m in range(M)]), "cuda")


def _epilogue_tiles(bits, m, M, temp, lse, step, table):
    """the keys [n_tiles] and statistics [n_tiles, 2] the lm_head epilogue leaves for the row `bits` at row index m of an M-row call"""
    ops = _ops()
    V = len(bits)
    nt = (V + 15) // 16
    w = torch.zeros((V, 32), dtype=BF16)
    w[:, 0] = _from_bits(bits)
    x = torch.zeros((M, 32), dtype=BF16, device="cuda")
    x[:, 0] = 1.0
    out = torch.empty((M, (V + 7) // 8 * 8 + 8), dtype=BF16, device="cuda")[:, :V]
    keys = torch.zeros((M, nt), dtype=torch.int64, device="cuda")
    stats = torch.zeros((M, nt, 2), dtype=torch.float32, device="cuda") if lse else None
    kw = dict(sample_rows=table) if table is not None else dict(sample=(temp, SEED, step) if temp > 0 else None)
    ops.gemm(x, ops.PackedLinear.from_weight(w.cuda()), out=out, argmax_partial=keys, lse_partial=stats, **kw)
    assert P.same_bits(_bits(out[m]), bits).all(), "the one-hot GEMM must reproduce the row"
    return keys[m].cpu().numpy(), stats[m].cpu().numpy().view(np.uint32) if lse else None


def _run(V, rows, temp=0.0, lse=False, keyed="scalar", n=None, fused=True, step_value=3, counted=None):
    """One kernel call over `rows` = [(History, fed token, size, logits bits)] and every check of it against the reference.  n: the
    scalar size (then every row's size is n), None: the sizes travel as row_n.  counted (a list): gets one entry per row checked, whether the
    row banned a column.  Returns the device logits, keys, statistics."""
    ops = _ops()
    M = len(rows)
    nt = (V + 15) // 16
    hists = [h.copy() for h, _, _, _ in rows]
    logits, logits_buf = _guarded(np.stack([bits for _, _, _, bits in rows]), BF16, 1.0)
    hist, hist_buf = _guarded(np.stack([h.hist for h in hists]), torch.int32, GUARD)
    hlen, hlen_buf = _guarded(np.array([h.len for h in hists], dtype=np.int32), torch.int32, GUARD)
    ids = torch.tensor([tok for _, tok, _, _ in rows], dtype=torch.int64, device="cuda")
    sizes = [size for _, _, size, _ in rows]
    row_n = None if n is not None else torch.tensor(sizes, dtype=torch.int32, device="cuda")
    keys = keys_buf = stats = stats_buf = None
    if fused:
        keys, keys_buf = _guarded(np.full((M, nt), KEY_FILL, dtype=np.int64), torch.int64, GUARD)
        if lse:
            stats, stats_buf = _guarded(np.full((M, nt, 2), STAT_FILL, dtype=np.float32), torch.float32, float(GUARD))
    step = torch.tensor([step_value], dtype=torch.int64, device="cuda")
    table = _table(M, temp) if keyed == "rows" else None
    table0 = None if table is None else table.clone()
    ops.logit_ngram_ban(logits, ids, hist, hlen, n=0 if n is None else n, row_n=row_n, temperature=0.0 if table is not None else temp,
                        seed=SEED, step=step, argmax_partial=keys, lse_partial=stats, sample_rows=table)
    torch.cuda.synchronize()
    got, got_hist, got_len = _bits(logits), hist.cpu().numpy(), hlen.cpu().numpy()
    got_keys = keys.cpu().numpy() if fused else None
    got_stats = stats.cpu().numpy().view(np.uint32) if lse and fused else None
    for m, (h0, tok, size, bits) in enumerate(rows):
        h = h0.copy()
        want, cols = R.step(bits, h, tok, size)
        if counted is not None:
            counted.append(bool(cols))
        assert np.array_equal(got_hist[m], h.hist) and got_len[m] == h.len, f"row {m}: the history record"
        bad = np.flatnonzero(got[m] != want)
        assert bad.size == 0, f"row {m} (n={size}): columns {bad[:8]} hold {got[m][bad[:8]]}, the reference {want[bad[:8]]}"
        if not fused:
            continue
        touched = sorted({c // 16 for c in cols})
        rest = np.setdiff1d(np.arange(nt), touched)
        assert (got_keys[m][rest] == KEY_FILL).all(), f"row {m}: a key outside the banned columns' tiles was written"
        if lse:
            assert (got_stats[m][rest] == np.float32(STAT_FILL).view(np.uint32)).all(), f"row {m}: statistics outside the banned tiles"
        if touched:
            ek, es = _epilogue_tiles(want, m, M, temp, lse, step, table0)
            assert np.array_equal(got_keys[m][touched], ek[touched]), f"row {m} T={temp}: keys of tiles {touched} are not the epilogue's"
            if lse:
                assert _same_words(got_stats[m][touched], es[touched]), f"row {m} T={temp}: statistics of tiles {touched}"
    assert float(logits_buf[-1]) == 1.0 and int(hist_buf[-1]) == GUARD and int(hlen_buf[-1]) == GUARD, "a guard word was written"
    if fused:
        assert int(keys_buf[-1]) == GUARD and (not lse or float(stats_buf[-1]) == GUARD), "a guard word was written"
    if table is not None:
        assert torch.equal(table, table0), "the kernel only reads the table"
    return logits, keys, stats


def _rows_of(V, cases, offset=0):
    return [(_case_history(c), c[2], c[3], _base_row(V, offset + i)) for i, c in enumerate(cases)]


# ----------------------------------------------------------------------------- 1. the crafted set, every mode and keying
@pytest.mark.parametrize("keyed", ["scalar", "rows"])
@pytest.mark.parametrize("temp,lse", MODES)
@pytest.mark.parametrize("V", [40, 330, 4112])
def test_crafted_histories_match_the_reference(V, temp, lse, keyed):
    """every crafted row, 64 to a call with the sizes as row_n (the last call is the remainder: an M that is no multiple of anything),
    then the rows of each size again at M = 8 with the scalar n, and one row alone.  Non-vacuity, counted on the rows this test itself
    checked on the device: at least half of them ban at least one column"""
    cases = _cases(V)
    counted = []
    for at in range(0, len(cases), 64):
        _run(V, _rows_of(V, cases[at:at + 64], at), temp, lse, keyed, counted=counted)
    for n in SIZES:
        mine = [(i, c) for i, c in enumerate(cases) if c[3] == n and "len=25" in c[0]][:8]
        _run(V, [(_case_history(c), c[2], n, _base_row(V, i)) for i, c in mine], temp, lse, keyed, n=n, counted=counted)
    i, c = next((i, c) for i, c in enumerate(cases) if c[0] == "n=3 len=256 periodic4")
    _run(V, [(_case_history(c), c[2], 3, _base_row(V, i))], temp, lse, keyed, n=3, counted=counted)
    print(f"V={V} T={temp} lse={lse} {keyed}: {sum(counted)} of {len(counted)} rows checked on the device banned")
    assert len(counted) >= len(cases) and 2 * sum(counted) >= len(counted)


def test_the_crafted_set_bans_on_at_least_half_of_its_rows():
    """non-vacuity of the crafted set itself, counted in the reference alone: the share of rows whose ban set is not empty (the share
    of the rows checked on the device is asserted where they are checked)"""
    for V in (40, 330, 4112):
        cases = _cases(V)
        banning = sum(bool(R.step(_base_row(V, i), _case_history(c), c[2], c[3])[1]) for i, c in enumerate(cases))
        print(f"V={V}: {banning} of {len(cases)} crafted rows ban at least one column")
        assert 2 * banning >= len(cases)
        assert all(R.step(_base_row(V, i), _case_history(c), c[2], c[3])[1] for i, c in enumerate(cases) if "periodic" in c[0] and "len=1000" in c[0])


def test_special_columns_and_empty_rows():
    """what the definition says about single columns, spelled out on the reference's rows (the device check is test 1's)"""
    V = 330
    a, b, c, d = _letters(V)
    by_name = {name: (i, (name, pre, tok, n)) for i, (name, pre, tok, n) in enumerate(_cases(V))}
    for name, cols in (("separator between the n-grams", [c]), ("separator in the suffix", []), ("out-of-range id in the suffix", []),
                       ("follower out of range", []), ("follower a separator", []), ("separator in the prefix only", [d]),
                       ("fed id beyond int32", []), ("fed id negative", []), ("n=1 with separators", [a, b, c]), ("n=2 overlap", [a]),
                       ("n=2 two followers one tile", [b, c]), ("off", []), ("off full", [])):
        i, case = by_name[name]
        h = _case_history(case)
        len0 = h.len
        want, got = R.step(_base_row(V, i), h, case[2], case[3])
        assert got == sorted(cols), name
        assert h.len == (len0 + 1 if len0 >= 0 else len0), name
    # a NaN column that is banned becomes -inf, a -inf column stays, on the device
    rows = [(R.History(HIST_LD, [a, d, a, b, a, c]), a, 2, _base_row(V, r)) for r in (1, 2)]
    assert rows[0][3][a] == NAN and rows[0][3][d] == NAN and rows[1][3][b] == NINF
    logits, _, _ = _run(V, rows, 0.0, True, n=2)
    got = _bits(logits)
    assert got[0][d] == NINF and got[0][a] == NAN, "a banned NaN becomes -inf, an unbanned NaN stays"
    assert got[1][b] == NINF and got[1][c] == NINF and got[1][d] == NINF


def test_full_history_switches_the_row_off():
    """hist_len == hist_ld at record time: the length word becomes UMV_NGRAM_FULL, nothing else of the row is written - and the row
    stays off at the next call; hist_ld - 1 still records and bans"""
    V = 330
    a, b, c, d = _letters(V)
    seq = [(a, b, c)[i % 3] for i in range(HIST_LD + 1)]
    full, last = R.History(HIST_LD, seq[:HIST_LD]), R.History(HIST_LD, seq[:HIST_LD - 1])
    rows = [(full, seq[HIST_LD], 3, _base_row(V, 0)), (last, seq[HIST_LD - 1], 3, _base_row(V, 3))]
    _run(V, rows, 0.0, True, n=3)
    h = full.copy()
    h.record(seq[HIST_LD])
    assert h.len == R.FULL
    _run(V, [(h, a, 3, _base_row(V, 0))], T, True, n=3)


def test_row_n_mix():
    """sizes {0, 1, 3, 17, -1} in one call over one history: 0, 17 and -1 record and ban nothing"""
    V = 330
    a, b, c, d = _letters(V)
    pre = [(a, b, c, d)[i % 4] for i in range(40)]
    rows = [(R.History(HIST_LD, pre), a, size, _base_row(V, 6)) for size in (0, 1, 3, 17, -1)]
    for temp, lse in MODES:
        _run(V, rows, temp, lse)
    assert [bool(R.step(r[3], r[0].copy(), r[1], r[2])[1]) for r in rows] == [False, True, True, False, False]


def test_unfused_use_records_and_bans_without_partials():
    V = 4112
    _run(V, _rows_of(V, _cases(V)[:64]), fused=False)


# ----------------------------------------------------------------------------- 2. batch independence
@pytest.mark.parametrize("V", [330, 4112])
def test_a_row_does_not_depend_on_its_batch(V):
    """a row inside an M = 64 call and the same row alone at M = 1: logits, keys and statistics bit for bit.  (A row's sampling key
    names the row in the scalar keying, so the lone sampled run is row 0's; with a table every row carries its own key.)"""
    cases = [c for c in _cases(V) if any(f"len={v} " in c[0] for v in (255, 256, 257, 1000))][:64]
    rows = _rows_of(V, cases)
    assert len(rows) == 64
    for temp in (0.0, T):
        many = _run(V, rows, temp, True)
        for i in ((0, 17, 63) if temp == 0 else (0,)):
            one = _run(V, rows[i:i + 1], temp, True)
            assert torch.equal(one[0].view(torch.int16), many[0][i:i + 1].view(torch.int16)) and torch.equal(one[1], many[1][i:i + 1]) \
                and torch.equal(one[2].view(torch.int32), many[2][i:i + 1].view(torch.int32)), f"row {i} T={temp}"


# ----------------------------------------------------------------------------- 3. picks against the independent entries
def _step_bufs(B, max_len, s):
    dev = "cuda"
    return dict(slot=torch.zeros(B, dtype=torch.int32, device=dev), pos=torch.zeros(B, dtype=torch.int32, device=dev),
                kvl=torch.ones(B, dtype=torch.int32, device=dev), ids=torch.full((B,), -5, dtype=torch.int64, device=dev),
                in_ids=torch.zeros((max_len, B), dtype=torch.int64, device=dev), pred=torch.zeros((max_len, B), dtype=torch.int64, device=dev),
                step=torch.full((B,), s, dtype=torch.int64, device=dev), lp=torch.zeros((max_len, B), dtype=torch.float32, device=dev))


@functools.lru_cache(maxsize=None)
def _problem(M, V):
    ops = _ops()
    K = 512
    g = torch.Generator().manual_seed(100 * M + V)
    x = torch.randn(M, K, generator=g).to(BF16).cuda()
    w = (torch.randn(V, K, generator=g) * (3.0 / K ** 0.5)).to(BF16).cuda()
    return x, ops.PackedLinear.from_weight(w)


def _lm_head(M, V, temp, lse, step):
    ops = _ops()
    x, lin = _problem(M, V)
    nt = (V + 15) // 16
    out = torch.empty((M, (V + 7) // 8 * 8 + 8), dtype=BF16, device="cuda")[:, :V]
    keys = torch.zeros((M, nt), dtype=torch.int64, device="cuda")
    stats = torch.zeros((M, nt, 2), dtype=torch.float32, device="cuda") if lse else None
    ops.gemm(x, lin, out=out, argmax_partial=keys, lse_partial=stats, sample=(temp, SEED, step) if temp > 0 else None)
    return out, keys, stats


def _banned_step(M, V, temp, lse, s=2):
    """a real lm_head call, then the kernel at n = 2 on a history in which the fed token was followed once by the row's raw argmax and
    once by its runner-up: both are banned"""
    ops = _ops()
    b = _step_bufs(M, 4, s)
    out, keys, stats = _lm_head(M, V, temp, lse, b["step"])
    top2 = out.float().topk(2, dim=-1).indices.tolist()
    raw = _bits(out)
    fed = [(5 * m + 1) % V for m in range(M)]
    hists = [R.History(64, [fed[m], top2[m][0], 7 % V, fed[m], top2[m][1], 9 % V]) for m in range(M)]
    hist = torch.from_numpy(np.stack([h.hist for h in hists])).cuda()
    hlen = torch.tensor([h.len for h in hists], dtype=torch.int32, device="cuda")
    ops.logit_ngram_ban(out, torch.tensor(fed, dtype=torch.int64, device="cuda"), hist, hlen, n=2, temperature=temp, seed=SEED,
                        step=b["step"], argmax_partial=keys, lse_partial=stats)
    for m in range(M):
        want, cols = R.step(raw[m], hists[m], fed[m], 2)
        assert set(top2[m]) <= set(cols) and np.array_equal(_bits(out[m]), want), f"row {m}: banned logits against the reference"
    return out, keys, stats, b, top2


@pytest.mark.parametrize("M", [1, 8, 64])
@pytest.mark.parametrize("V", [40, 330, 4112])
def test_fused_picks_equal_the_stand_alone_entries_on_the_banned_logits(V, M):
    ops = _ops()
    s = 2
    out, keys, _, b, top2 = _banned_step(M, V, 0.0, False, s)
    ops.decode_step_end_argmax(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"])
    assert torch.equal(b["ids"], ops.argmax(out)), "greedy"
    assert all(int(i) not in t for i, t in zip(b["ids"].tolist(), top2)), "a banned column was picked"
    out, keys, stats, b, _ = _banned_step(M, V, 0.0, True, s)
    ops.decode_step_end_logprob(b["slot"], b["pos"], b["kvl"], keys, stats, b["ids"], b["in_ids"], b["pred"], b["step"], out, b["lp"], 0.0)
    alone = ops.token_logprob(out, b["ids"], 0.0)
    bits = _bits(out)
    model = torch.tensor([P.logprob(bits[m], int(b["ids"][m])) for m in range(M)])
    d1, d2 = float((b["lp"][s] - alone).abs().max()), float((b["lp"][s].cpu().double() - model).abs().max())
    print(f"V={V} M={M}: logprob vs stand-alone {d1:.3g}, vs fp64 {d2:.3g}")
    assert d1 <= BOUND and d2 <= BOUND
    out, keys, _, b, top2 = _banned_step(M, V, T, False, s)
    st = b["step"][:1].clone()
    ops.decode_step_end_argmax(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"])
    assert torch.equal(b["ids"], ops.sample(out, T, SEED, step=st)), "sampling"
    assert all(int(i) not in t for i, t in zip(b["ids"].tolist(), top2)), "a banned column was sampled"
    out, keys, stats, b, _ = _banned_step(M, V, T, True, s)
    ops.decode_step_end_logprob(b["slot"], b["pos"], b["kvl"], keys, stats, b["ids"], b["in_ids"], b["pred"], b["step"], out, b["lp"], T)
    lp = ops.token_logprob(out, b["ids"], T)
    assert float((b["lp"][s] - lp).abs().max()) <= BOUND, "sampled log-probability of the banned, renormalised softmax"


def test_six_steps_feeding_the_pick_back():
    """lm_head, ban, greedy step end, six times over, each step fed the previous pick: logits and history follow the reference, every
    pick is the stand-alone argmax of the banned logits, and with n = 1 no row is fed a token twice"""
    ops = _ops()
    V, M = 330, 8
    for n in (1, 2):
        b = _step_bufs(M, 8, 0)
        hists = [R.History(16) for _ in range(M)]
        hist = torch.zeros((M, 16), dtype=torch.int32, device="cuda")
        hlen = torch.zeros(M, dtype=torch.int32, device="cuda")
        b["ids"][:] = torch.arange(M) % 3          # the start tokens
        fed = [[] for _ in range(M)]
        for s in range(6):
            out, keys, _ = _lm_head(M, V, 0.0, False, None)      # (the same logits every step: at n = 1 each step must move on)
            raw = _bits(out)
            ids = b["ids"].tolist()
            ops.logit_ngram_ban(out, b["ids"], hist, hlen, n=n, argmax_partial=keys)
            for m in range(M):
                fed[m].append(ids[m])
                want, _ = R.step(raw[m], hists[m], ids[m], n)
                assert np.array_equal(_bits(out[m]), want), f"n={n} step {s} row {m}"
            assert np.array_equal(hist.cpu().numpy(), np.stack([h.hist for h in hists])) and hlen.tolist() == [h.len for h in hists]
            ops.decode_step_end_argmax(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"])
            assert torch.equal(b["ids"], ops.argmax(out)), f"n={n} step {s}"
        if n == 1:
            assert all(len(set(f + [t])) == 7 for f, t in zip(fed, b["ids"].tolist())), "n = 1: a token was fed twice"


# ----------------------------------------------------------------------------- 4. arguments
def test_rejected_arguments_launch_nothing():
    ops = _ops()
    from unimedvl_amd._lib import UmvError
    V = 40
    logits = torch.zeros((1, V), dtype=BF16, device="cuda")
    ids = torch.full((1,), 3, dtype=torch.int64, device="cuda")
    hist = torch.full((1, 8), 3, dtype=torch.int32, device="cuda")
    hlen = torch.full((1,), 4, dtype=torch.int32, device="cuda")
    keys = torch.zeros((1, 3), dtype=torch.int64, device="cuda")
    stats = torch.zeros((1, 3, 2), dtype=torch.float32, device="cuda")
    from unimedvl_amd import sampling
    table = sampling.to_tensor(sampling.pack([sampling.SamplingParams()]), "cuda")
    for kw in (dict(n=-1), dict(n=17), dict(temperature=-0.5), dict(temperature=float("nan")), dict(temperature=float("inf")),
               dict(lse_partial=stats), dict(argmax_partial=torch.zeros((1, 4), dtype=torch.int64, device="cuda")),
               dict(argmax_partial=keys, sample_rows=table, temperature=0.7),
               dict(row_n=torch.zeros(2, dtype=torch.int32, device="cuda"))):
        with pytest.raises(UmvError):
            ops.logit_ngram_ban(logits, ids, hist, hlen, **dict(dict(n=1), **kw))
    with pytest.raises(UmvError):
        ops.logit_ngram_ban(logits, ids, hist[:, :0].contiguous(), hlen, n=1)             # hist_ld < 1
    with pytest.raises(UmvError):
        ops.logit_ngram_ban(logits, ids[:0], hist, hlen, n=1)
    torch.cuda.synchronize()
    assert int(hlen[0]) == 4 and (logits == 0).all() and (hist == 3).all(), "a rejected call launched"
    ops.logit_ngram_ban(logits, ids, hist, hlen, n=1, argmax_partial=keys, lse_partial=stats)
    assert int(hlen[0]) == 5 and _bits(logits)[0][3] == NINF and int((logits[0] == 0).sum()) == V - 1
