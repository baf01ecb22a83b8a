"""umv_logit_sequence_ban_bf16 (include/unimedvl_hip.h, "banned sequences") at kernel level, bit for bit against the plain-Python
definition (tests/sequence_ban_ref.py): the banned logits, the count and tail record, the recomputed tiles against the lm_head epilogue
itself, the words nothing may touch, the picks of the fused step ends against the stand-alone entries, batch independence, the beam
form over crafted back-pointers and the argument checks.

The devices are tests/test_ngram_gpu.py's (the one-hot GEMM that makes the epilogue leave its keys and statistics for a given row, the
guarded buffers, the per-row table, the step buffers): imported, not copied.  The only tolerance is the header's 1e-4 on a
log-probability."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import penalty_ref as P
import sequence_ban_ref as R
import test_ngram_gpu as G
from test_ngram_gpu import BF16, BOUND, GUARD, KEY_FILL, MODES, NAN, NINF, SEED, STAT_FILL, T, _bits, _guarded, _ops, _same_words

pytestmark = pytest.mark.gpu
CHAIN = list(range(20, 35))             # the 15 distinct tokens the long entries are made of
TARGET = [(7 * m) % 32 for m in range(1, 17)]      # entry m's banned column: 16 distinct columns, 3 and 17 among them


@functools.lru_cache(maxsize=None)
def _crafted_table(V):
    """entries of every length 1..16 that end CHAIN's suffixes (a tail of CHAIN matches all of them, a tail that breaks at position p
    only the shorter ones); two entries that ban one column (18), which shares a tile with entry 7's (17); an entry into the ragged
    last tile; a last token and a first token outside the vocabulary; single tokens that hold until count 1 / 3 and by row_min"""
    table = [([7], 2)] + [(CHAIN[15 - (m - 1):] + [TARGET[m - 1]], 0) for m in range(2, 17)]
    assert TARGET[6] == 17 and TARGET[4] == 3
    table += [([34, 18], 0), ([33, 34, 18], 0), ([34, V - 1], 0), ([34, V + 5], 0), ([V + 2, 1], 0), ([38], 1), ([37], 3), ([36], R.ROW)]
    return table


@functools.lru_cache(maxsize=None)
def _crafted_rows(V):
    """[(name, State before the call, fed token, row_min)] - 64 of them"""
    rows = []
    for m in range(1, 17):                                   # a match at every length: the tail breaks just before the m - 1 tokens
        fed = [5] * (16 - m) + CHAIN[15 - (m - 1):]
        rows.append((f"match m={m}", R.State(fed[:-1], count=1 if m == 1 else None), fed[-1], 0))
    for p in range(15):                                      # a near miss at each position of the longest entry
        fed = list(CHAIN)
        fed[p] = 6
        rows.append((f"near miss at {p}", R.State(fed[:-1]), fed[-1], 0))
    rows += [
        ("the whole chain", R.State(CHAIN[:-1]), CHAIN[-1], 0),                 # all lengths, 17 + 18 in one tile, V - 1
        ("chain, too few fed", R.State(CHAIN[:-1], count=7), CHAIN[-1], 0),     # m - 1 <= count: only the entries up to m = 9
        ("off", R.State(CHAIN[:-1], count=-1), CHAIN[-1], 5),
        ("off, second", R.State([33], count=-7), 34, 5),
        ("first token out of range", R.State([5]), V + 2, 0),
        ("fed id beyond int32", R.State([33]), (1 << 31) + 34, 0),
        ("fed id negative", R.State([33]), -(1 << 40), 0),
        ("count 1: begin entries", R.State(), 9, 0),
        ("count 3: until 3 holds", R.State([9, 9]), 9, 0),
        ("count 4: until 3 is over", R.State([9, 9, 9]), 9, 0),
        ("row_min 0", R.State(), 9, 0),
        ("row_min 1 at count 1", R.State(), 9, 1),
        ("row_min 2 at count 3", R.State([9, 9]), 9, 2),
        ("row_min 3 at count 3", R.State([9, 9]), 9, 3),
        ("row_min 100", R.State([9] * 40), 9, 100),
        ("row_min negative", R.State([9]), 9, -4),
        ("count saturates", R.State([33], count=R.COUNT_MAX), 34, 0),
    ]
    rng = np.random.default_rng(V)
    while len(rows) < 64:                                    # random walks over the chain's tokens: mostly nothing to ban
        fed = rng.integers(28, 36, int(rng.integers(1, 30))).tolist()
        rows.append((f"random {len(rows)}", R.State(fed[:-1]), fed[-1], int(rng.integers(0, 4))))
    return rows


def _base_row(V, r, name=""):
    """test_ngram_gpu's rows - N(0, 3^2), in turn a NaN or a -inf on columns 3 / V - 1 and 17 / 18; an off row is all NaN"""
    bits = G._base_row(V, r)
    if name.startswith("off"):
        bits[:] = NAN
    return bits


def _run(V, rows, table, temp=0.0, lse=False, keyed="scalar", fused=True, step_value=3, counted=None):
    """One plain-form kernel call over `rows` = [(State, fed token, row_min, logits bits)] and every check of it against the
    reference.  Returns the device logits, keys, statistics."""
    ops = _ops()
    M, nt = len(rows), (V + 15) // 16
    ptr, tok, until = [0], [], []
    for w, u in table:
        tok += w
        ptr.append(len(tok))
        until.append(u)
    dev_table = ops.SequenceTable(ptr, tok, until, "cuda")
    logits, logits_buf = _guarded(np.stack([bits for _, _, _, bits in rows]), BF16, 1.0)
    tail, tail_buf = _guarded(np.stack([s.tail for s, _, _, _ in rows]), torch.int32, GUARD)
    count, count_buf = _guarded(np.array([s.count for s, _, _, _ in rows], dtype=np.int32), torch.int32, GUARD)
    row_min = torch.tensor([rm for _, _, rm, _ in rows], dtype=torch.int32, device="cuda")
    ids = torch.tensor([t for _, t, _, _ in rows], dtype=torch.int64, device="cuda")
    keys = keys_buf = stats = stats_buf = None
    if fused:
        keys, keys_buf = _guarded(np.full((M, nt), KEY_FILL, dtype=np.int64), torch.int64, GUARD)
        if lse:
            stats, stats_buf = _guarded(np.full((M, nt, 2), STAT_FILL, dtype=np.float32), torch.float32, float(GUARD))
    step = torch.tensor([step_value], dtype=torch.int64, device="cuda")
    rows_table = G._table(M, temp) if keyed == "rows" else None
    rows_table0 = None if rows_table is None else rows_table.clone()
    ops.logit_sequence_ban(logits, ids, dev_table, tail=tail, count=count, row_min=row_min, temperature=0.0 if rows_table is not None else temp,
                           seed=SEED, step=step, argmax_partial=keys, lse_partial=stats, sample_rows=rows_table)
    torch.cuda.synchronize()
    got, got_tail, got_count = _bits(logits), tail.cpu().numpy(), count.cpu().numpy()
    got_keys = keys.cpu().numpy() if fused else None
    got_stats = stats.cpu().numpy().view(np.uint32) if lse and fused else None
    for m, (s0, fed, rm, bits) in enumerate(rows):
        s = s0.copy()
        want, cols = R.step(bits, s, fed, table, rm)
        if counted is not None:
            counted.append(bool(cols))
        assert np.array_equal(got_tail[m], s.tail) and got_count[m] == s.count, f"row {m}: the record (count {got_count[m]} / {s.count})"
        bad = np.flatnonzero(got[m] != want)
        assert bad.size == 0, f"row {m}: columns {bad[:8]} hold {got[m][bad[:8]]}, the reference {want[bad[:8]]} (banned {cols})"
        if not fused:
            continue
        touched = sorted({c // 16 for c in cols})
        rest = np.setdiff1d(np.arange(nt), touched)
        assert (got_keys[m][rest] == KEY_FILL).all(), f"row {m}: a key outside the banned columns' tiles was written"
        if lse:
            assert (got_stats[m][rest] == np.float32(STAT_FILL).view(np.uint32)).all(), f"row {m}: statistics outside the banned tiles"
        if touched:
            ek, es = G._epilogue_tiles(want, m, M, temp, lse, step, rows_table0)
            assert np.array_equal(got_keys[m][touched], ek[touched]), f"row {m} T={temp}: keys of tiles {touched} are not the epilogue's"
            if lse:
                assert _same_words(got_stats[m][touched], es[touched]), f"row {m} T={temp}: statistics of tiles {touched}"
    assert float(logits_buf[-1]) == 1.0 and int(tail_buf[-1]) == GUARD and int(count_buf[-1]) == GUARD, "a guard word was written"
    if fused:
        assert int(keys_buf[-1]) == GUARD and (not lse or float(stats_buf[-1]) == GUARD), "a guard word was written"
    if rows_table is not None:
        assert torch.equal(rows_table, rows_table0), "the kernel only reads the table"
    return logits, keys, stats


def _rows_of(V, crafted, offset=0):
    return [(s, fed, rm, _base_row(V, offset + i, name)) for i, (name, s, fed, rm) in enumerate(crafted)]


# ----------------------------------------------------------------------------- 1. the crafted set, every mode and keying
def test_the_crafted_set_is_a_condition():
    """asserted on the reference alone: at least half of the rows ban, at least one bans nothing, and the named cases do what their
    names say"""
    for V in (40, 330, 4112):
        table, crafted = _crafted_table(V), _crafted_rows(V)
        assert len(crafted) == 64
        cols = {}
        for i, (name, s0, fed, rm) in enumerate(crafted):
            s = s0.copy()
            cols[name] = R.step(_base_row(V, i, name), s, fed, table, rm)[1]
        banning = sum(bool(c) for c in cols.values())
        print(f"V={V}: {banning} of {len(crafted)} crafted rows ban at least one column")
        assert 2 * banning >= len(crafted) and banning < len(crafted)
        assert cols["match m=1"] == [7, 37]                  # (count 2: the single tokens that hold until 2 and 3)
        for m in range(2, 17):                               # (a tail that ends on 34 also completes the words into 18 and V - 1)
            assert cols[f"match m={m}"] == sorted(set(TARGET[1:m]) | {18, V - 1}), f"match m={m}"
        for p in range(14):
            assert cols[f"near miss at {p}"] == sorted(set(TARGET[1:15 - p]) | {18, V - 1}), f"near miss at {p}"
        assert cols["near miss at 14"] == []
        assert {17, 18, V - 1} <= set(cols["the whole chain"]) and len(cols["the whole chain"]) == 17
        assert set(cols["chain, too few fed"]) & set(TARGET) == set(TARGET[1:9])
        assert cols["off"] == cols["off, second"] == []
        assert cols["first token out of range"] == cols["fed id beyond int32"] == cols["fed id negative"] == [7, 37]
        assert cols["count 1: begin entries"] == [7, 37, 38]
        assert cols["count 3: until 3 holds"] == [37] and cols["count 4: until 3 is over"] == []
        assert cols["row_min 0"] == [7, 37, 38] and cols["row_min 1 at count 1"] == [7, 36, 37, 38]
        assert cols["row_min 2 at count 3"] == [37] and cols["row_min 3 at count 3"] == [36, 37] and cols["row_min 100"] == [36]
        assert cols["row_min negative"] == [7, 37] and cols["count saturates"] == [14, 18, 21, V - 1]


@pytest.mark.parametrize("keyed", ["scalar", "rows"])
@pytest.mark.parametrize("temp,lse", MODES)
@pytest.mark.parametrize("V", [40, 330, 4112])
def test_crafted_rows_match_the_reference(V, temp, lse, keyed):
    """the 64 crafted rows in one call, eight of them at M = 8, one alone: logits, keys, statistics, tail and count bit for bit; the
    rows this test checked on the device ban on at least half of them"""
    table, crafted = _crafted_table(V), _crafted_rows(V)
    counted = []
    _run(V, _rows_of(V, crafted), table, temp, lse, keyed, counted=counted)
    _run(V, _rows_of(V, crafted[12:20], 12), table, temp, lse, keyed, counted=counted)
    _run(V, _rows_of(V, crafted[31:32], 31), table, temp, lse, keyed, counted=counted)
    assert len(counted) == 73 and 2 * sum(counted) >= len(counted) and sum(counted) < len(counted)


def test_special_columns_on_the_device():
    """a banned NaN becomes -inf, an unbanned NaN stays, a -inf stays; an off row - all NaN, between two rows that ban - keeps every
    bit; the same rows on the unfused step (no keys, no statistics)"""
    V = 330
    table, crafted = _crafted_table(V), _crafted_rows(V)
    by_name = {name: i for i, (name, _, _, _) in enumerate(crafted)}
    pick = [by_name["the whole chain"], by_name["off"], by_name["match m=16"]]
    rows = [(crafted[i][1], crafted[i][2], crafted[i][3], _base_row(V, r, crafted[i][0])) for i, r in zip(pick, (1, 0, 2))]
    assert rows[0][3][3] == NAN and rows[0][3][V - 1] == NAN and rows[2][3][17] == NINF and (rows[1][3] == NAN).all()
    for fused in (True, False):
        logits, _, _ = _run(V, rows, table, 0.0, True, fused=fused)
        got = _bits(logits)
        assert got[0][3] == NINF and got[0][V - 1] == NINF and got[2][17] == NINF and (got[1] == NAN).all()
    _run(V, _rows_of(V, crafted), table, fused=False)
    bits = _base_row(4112, 1)
    bits[5] = NAN
    logits, _, _ = _run(4112, [(R.State(), 9, 0, bits)], _crafted_table(4112), T, True)
    assert _bits(logits)[0][5] == NAN, "an unbanned NaN stays"


def test_an_empty_table_records_only():
    V = 40
    crafted = _crafted_rows(V)
    for fused in (True, False):
        _run(V, _rows_of(V, crafted[:8]), [], 0.0, fused, fused=fused)


# ----------------------------------------------------------------------------- 2. batch independence
@pytest.mark.parametrize("V", [330, 4112])
def test_a_row_does_not_depend_on_its_batch(V):
    """a row inside the M = 64 call and the same row alone at M = 1: logits, keys and statistics bit for bit.  (A row's sampling key
    names the row in the scalar keying, so the lone sampled run is row 0's.)"""
    table, rows = _crafted_table(V), _rows_of(V, _crafted_rows(V))
    for temp in (0.0, T):
        many = _run(V, rows, table, temp, True)
        for i in ((0, 15, 31, 63) if temp == 0 else (0,)):
            one = _run(V, [(rows[i][0], rows[i][1], rows[i][2], rows[i][3])], table, temp, True)
            assert torch.equal(one[0].view(torch.int16), many[0][i:i + 1].view(torch.int16)) and torch.equal(one[1], many[1][i:i + 1]) \
                and torch.equal(one[2].view(torch.int32), many[2][i:i + 1].view(torch.int32)), f"row {i} T={temp}"


# ----------------------------------------------------------------------------- 3. picks against the independent entries
def _dev_table(table):
    ops = _ops()
    ptr, tok = [0], []
    for w, _ in table:
        tok += w
        ptr.append(len(tok))
    return ops.SequenceTable(ptr, tok, [u for _, u in table], "cuda")


def _banned_step(M, V, temp, lse, s=2):
    """a real lm_head call, then the kernel with a table that bans every row's raw argmax and its runner-up after the fed token
    (two-token words) and column V - 2 while count <= row_min"""
    ops = _ops()
    b = G._step_bufs(M, 4, s)
    out, keys, stats = G._lm_head(M, V, temp, lse, b["step"])
    top2 = out.float().topk(2, dim=-1).indices.tolist()
    raw = _bits(out)
    fed = [(5 * m + 1) % V for m in range(M)]
    table = [([fed[m], top2[m][j]], 0) for m in range(M) for j in (0, 1)] + [([V - 2], R.ROW)]
    states = [R.State([9]) for _ in range(M)]
    tail = torch.from_numpy(np.stack([st.tail for st in states])).cuda()
    count = torch.tensor([st.count for st in states], dtype=torch.int32, device="cuda")
    row_min = torch.full((M,), 2, dtype=torch.int32, device="cuda")
    ops.logit_sequence_ban(out, torch.tensor(fed, dtype=torch.int64, device="cuda"), _dev_table(table), tail=tail, count=count,
                           row_min=row_min, temperature=temp, seed=SEED, step=b["step"], argmax_partial=keys, lse_partial=stats)
    for m in range(M):
        want, cols = R.step(raw[m], states[m], fed[m], table, 2)
        assert set(top2[m]) | {V - 2} <= set(cols) and np.array_equal(_bits(out[m]), want), f"row {m}: banned logits against the reference"
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
    """lm_head, ban, greedy step end, six times over the same logits, each step fed the previous pick.  The table bans every pick of
    the unbanned chain after its predecessor, the raw argmax while count <= row_min = 3 and column 0 at the first step: logits, tail
    and count follow the reference, every pick is the stand-alone argmax of the banned logits"""
    ops = _ops()
    V, M = 330, 8
    out0, _, _ = G._lm_head(M, V, 0.0, False, None)
    best = out0.float().argmax(-1).tolist()
    table = [([m % 3, best[m]], 0) for m in range(M)] + [([best[m], best[m]], 0) for m in range(M)] + \
        [([best[m]], R.ROW) for m in range(M)] + [([0], 1)]
    dev_table = _dev_table(table)
    b = G._step_bufs(M, 8, 0)
    states = [R.State() for _ in range(M)]
    tail = torch.full((M, R.TAIL), -1, dtype=torch.int32, device="cuda")
    count = torch.zeros(M, dtype=torch.int32, device="cuda")
    row_min = torch.tensor([m % 5 for m in range(M)], dtype=torch.int32, device="cuda")
    b["ids"][:] = torch.arange(M) % 3          # the start tokens
    banned_steps = 0
    for s in range(6):
        out, keys, _ = G._lm_head(M, V, 0.0, False, None)
        raw = _bits(out)
        ids = b["ids"].tolist()
        ops.logit_sequence_ban(out, b["ids"], dev_table, tail=tail, count=count, row_min=row_min, argmax_partial=keys)
        for m in range(M):
            want, cols = R.step(raw[m], states[m], ids[m], table, m % 5)
            banned_steps += bool(cols)
            assert np.array_equal(_bits(out[m]), want), f"step {s} row {m}"
        assert np.array_equal(tail.cpu().numpy(), np.stack([st.tail for st in states])) and count.tolist() == [st.count for st in states]
        ops.decode_step_end_argmax(b["slot"], b["pos"], b["kvl"], keys, b["ids"], b["in_ids"], b["pred"], b["step"])
        assert torch.equal(b["ids"], ops.argmax(out)), f"step {s}"
    assert banned_steps >= 12 and count.tolist() == [6] * M


# ----------------------------------------------------------------------------- 4. the beam form
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("K", [2, 3, 10])
def test_beam_form_matches_the_reference(K, B):
    """crafted back-pointers - random, one step of swaps, one with all children of one parent - at t in {0, 1, 5, 20} and max_m in
    {1, 2, 16}: tokens come from a small alphabet, the table holds words that the walks complete, until entries and a row_min mix.
    Logits, keys and statistics bit for bit; no state is written"""
    ops = _ops()
    V, max_len = 330, 24
    Rn = B * K
    nt = (V + 15) // 16
    rng = np.random.default_rng(10 * K + B)
    tok = rng.integers(20, 23, (max_len, Rn)).astype(np.int32)
    par = rng.integers(0, K, (max_len, Rn)).astype(np.int32)
    par[3] = np.tile(np.arange(K)[::-1], B)                  # swaps
    par[4] = 1                                               # all children of one parent
    par[18] = np.tile(np.roll(np.arange(K), 1), B)
    starts = [21, 22][:B]
    checked = banned = 0
    for max_m in (1, 2, 16):
        words = [([37], 2), ([36], R.ROW), ([38], 0)]
        if max_m >= 2:
            words += [([a, 40 + a], 0) for a in (20, 21, 22)]
        if max_m == 16:
            words += [([a, c, 60 + 3 * (a - 20) + (c - 20)], 0) for a in (20, 21, 22) for c in (20, 21, 22)]
            words += [([21, a, c, d, 80 + (a + c + d) % 9], 0) for a in (20, 21) for c in (20, 21, 22) for d in (20, 22)]
            words += [([20] * 15 + [99], 0)]
        table = words
        dev_table = _dev_table(table)
        assert dev_table.max_m == max_m
        for t in (0, 1, 5, 20):
            fed = [starts[r // K] if t == 0 else int(tok[t - 1, r]) for r in range(Rn)]
            rows = [_base_row(V, 7 * t + r) for r in range(Rn)]
            logits, logits_buf = _guarded(np.stack(rows), BF16, 1.0)
            keys, keys_buf = _guarded(np.full((Rn, nt), KEY_FILL, dtype=np.int64), torch.int64, GUARD)
            stats, stats_buf = _guarded(np.full((Rn, nt, 2), STAT_FILL, dtype=np.float32), torch.float32, float(GUARD))
            d_tok, d_par = torch.from_numpy(tok).cuda(), torch.from_numpy(par).cuda()
            step_idx = torch.full((Rn,), t, dtype=torch.int64, device="cuda")
            row_min = torch.tensor([(3 * r) % 7 for r in range(Rn)], dtype=torch.int32, device="cuda")
            ops.logit_sequence_ban(logits, torch.tensor(fed, dtype=torch.int64, device="cuda"), dev_table, row_min=row_min,
                                   beam=(d_tok, d_par, step_idx, torch.tensor(starts, dtype=torch.int64, device="cuda"), K),
                                   argmax_partial=keys, lse_partial=stats)
            torch.cuda.synchronize()
            got, got_keys, got_stats = _bits(logits), keys.cpu().numpy(), stats.cpu().numpy().view(np.uint32)
            for r in range(Rn):
                want, cols = R.beam_step(rows[r], tok, par, t, r, K, fed[r], starts[r // K], table, dev_table.max_m, (3 * r) % 7)
                checked += 1
                banned += len(cols) > 1                       # (column 38 is banned everywhere)
                assert np.array_equal(got[r], want), f"K={K} max_m={max_m} t={t} row {r}: banned {cols}"
                touched = sorted({c // 16 for c in cols})
                rest = np.setdiff1d(np.arange(nt), touched)
                assert (got_keys[r][rest] == KEY_FILL).all() and (got_stats[r][rest] == np.float32(STAT_FILL).view(np.uint32)).all()
                ek, es = G._epilogue_tiles(want, r, Rn, 0.0, True, None, None)
                assert np.array_equal(got_keys[r][touched], ek[touched]) and _same_words(got_stats[r][touched], es[touched])
            assert float(logits_buf[-1]) == 1.0 and int(keys_buf[-1]) == GUARD and float(stats_buf[-1]) == GUARD
            assert torch.equal(d_tok.cpu(), torch.from_numpy(tok)) and torch.equal(d_par.cpu(), torch.from_numpy(par))
            assert step_idx.tolist() == [t] * Rn
    print(f"K={K} B={B}: {banned} of {checked} rows ban beyond the suppressed column")
    assert 3 * banned >= checked


def test_beam_form_follows_the_long_walk():
    """max_m = 16 at t = 20: a word made of the 14 tokens the walk from row 0 reads, the fed token and a last one is banned for row 0
    and only there; a step counter outside [0, max_len) bans nothing"""
    ops = _ops()
    V, K, max_len = 330, 3, 24
    rng = np.random.default_rng(5)
    tok = rng.integers(20, 30, (max_len, K)).astype(np.int32)
    par = rng.integers(0, K, (max_len, K)).astype(np.int32)
    t = 20
    count, tail = R.beam_state(tok, par, t, 0, K, int(tok[t - 1, 0]), 21, 16)
    assert count == 21 and (tail >= 0).all()
    table = [(tail.tolist() + [111], 0)]
    dev_table = _dev_table(table)
    fed = [int(tok[t - 1, r]) for r in range(K)]
    for tt in (t, max_len, -1):
        rows = [_base_row(V, r) for r in range(K)]
        logits = G._from_bits(np.stack(rows)).cuda()
        ops.logit_sequence_ban(logits, torch.tensor(fed, dtype=torch.int64, device="cuda"), dev_table,
                               beam=(torch.from_numpy(tok).cuda(), torch.from_numpy(par).cuda(),
                                     torch.full((K,), tt, dtype=torch.int64, device="cuda"), torch.tensor([21], dtype=torch.int64, device="cuda"), K))
        got = _bits(logits)
        cols = [R.beam_step(rows[r], tok, par, tt, r, K, fed[r], 21, table, 16)[1] for r in range(K)]
        assert cols[0] == ([111] if tt == t else []) and (tt == t or cols == [[], [], []])
        for r in range(K):
            assert np.array_equal(got[r], R.ban_row(rows[r], cols[r])), f"t={tt} row {r}"


# ----------------------------------------------------------------------------- 5. arguments
def test_rejected_arguments_launch_nothing():
    ops = _ops()
    from unimedvl_amd import _lib, sampling
    from unimedvl_amd._lib import UmvError
    V = 40
    logits = torch.zeros((2, V), dtype=BF16, device="cuda")
    ids = torch.full((2,), 3, dtype=torch.int64, device="cuda")
    tail = torch.full((2, R.TAIL), 3, dtype=torch.int32, device="cuda")
    count = torch.full((2,), 4, dtype=torch.int32, device="cuda")
    keys = torch.zeros((2, 3), dtype=torch.int64, device="cuda")
    stats = torch.zeros((2, 3, 2), dtype=torch.float32, device="cuda")
    rows = sampling.to_tensor(sampling.pack([sampling.SamplingParams()] * 2), "cuda")
    table = _dev_table([([3, 5], 0)])
    beam = (torch.zeros((4, 2), dtype=torch.int32, device="cuda"), torch.zeros((4, 2), dtype=torch.int32, device="cuda"),
            torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), 2)
    plain = dict(tail=tail, count=count)
    for kw in (dict(plain, temperature=-0.5), dict(plain, temperature=float("nan")), dict(plain, temperature=float("inf")),
               dict(plain, lse_partial=stats), dict(plain, argmax_partial=torch.zeros((2, 4), dtype=torch.int64, device="cuda")),
               dict(plain, argmax_partial=keys, sample_rows=rows, temperature=0.7), dict(tail=tail), dict(count=count), dict(),
               dict(plain, row_min=torch.zeros(3, dtype=torch.int32, device="cuda")), dict(tail=tail[:, :14].contiguous(), count=count),
               dict(plain, beam=beam), dict(beam=beam[:4] + (0,)), dict(beam=beam[:4] + (11,)), dict(beam=beam[:4] + (3,)),
               dict(beam=beam, argmax_partial=keys, sample_rows=rows), dict(beam=(beam[0], beam[1][:3].contiguous()) + beam[2:])):
        with pytest.raises(UmvError):
            ops.logit_sequence_ban(logits, ids, table, **kw)
    with pytest.raises(UmvError):
        ops.logit_sequence_ban(logits, ids[:1], table, **plain)
    with pytest.raises(ValueError):
        ops.SequenceTable([0, 17], list(range(17)), [0], "cuda")
    with pytest.raises(ValueError):
        ops.SequenceTable([0, 0], [], [0], "cuda")
    # the entry itself, past the wrapper's checks: a struct field at a time
    lib = _lib.load()

    def args(**kw):
        a = _lib.SequenceBanArgs()
        a.logits, a.ld, a.ids, a.M, a.V = logits.data_ptr(), V, ids.data_ptr(), 2, V
        a.seq_ptr, a.seq_tok, a.seq_until, a.S, a.n_tok, a.max_m = table.ptr.data_ptr(), table.tok.data_ptr(), table.until.data_ptr(), 1, 2, 2
        a.tail, a.count = tail.data_ptr(), count.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    b_tok, b_par, b_step, b_start, _ = beam
    beam_kw = dict(tail=None, count=None, beam_tok=b_tok.data_ptr(), beam_parent=b_par.data_ptr(), step_idx=b_step.data_ptr(),
                   start_ids=b_start.data_ptr(), K=2, max_len=4)
    for kw in (dict(S=-1), dict(S=_lib.SEQ_ENTRIES_MAX + 1), dict(seq_ptr=None), dict(seq_tok=None), dict(seq_until=None), dict(n_tok=0),
               dict(n_tok=17), dict(max_m=0), dict(max_m=17), dict(ids=None), dict(tail=None), dict(count=None), dict(ld=V - 1),
               dict(K=-1), dict(K=2), dict(beam_kw, K=11), dict(beam_kw, beam_tok=None), dict(beam_kw, beam_parent=None),
               dict(beam_kw, step_idx=None), dict(beam_kw, start_ids=None), dict(beam_kw, M=1), dict(beam_kw, max_len=0),
               dict(beam_kw, rows=rows.data_ptr(), argmax_partial=keys.data_ptr(), n_tiles=3)):
        assert lib.umv_logit_sequence_ban_bf16(C.byref(args(**kw)), None) == -1, f"{kw}: UMV_ERR_ARG expected"
    torch.cuda.synchronize()
    assert count.tolist() == [4, 4] and (logits == 0).all() and (tail == 3).all(), "a rejected call launched"
    ops.logit_sequence_ban(logits, ids, table, argmax_partial=keys, lse_partial=stats, **plain)
    assert count.tolist() == [5, 5] and _bits(logits)[0][5] == NINF and int((logits[0] == 0).sum()) == V - 1
