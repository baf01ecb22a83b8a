"""The banned-sequence stage without a GPU (include/unimedvl_hip.h, "banned sequences"): the plain-Python definition
(tests/sequence_ban_ref.py) against the four `transformers` processors it stands for, its edge cases, the table builder and the value
checks of ops.py, the beam form's walk against the plain history of the reconstructed sequence, and the keyword surface."""
import inspect

import numpy as np
import pytest

import sequence_ban_ref as R
from unimedvl_amd import ops

V = 50


# ----------------------------------------------------------------------------- 1. the reference is HF's four processors
def test_reference_equals_the_transformers_processors():
    """300 random sequences of 8 steps: input ids equal to the fed tokens (no prompt), the banned set of every step equal to the
    columns the four processors, applied in turn to a zero row, leave at -inf.  The start token is one no bad word holds, as a
    start token is: HF skips a word that is longer than its whole input, the definition here (m - 1 <= count) bans its last token
    when the fed tokens ARE its first m - 1 - with a prompt in HF's input that length rule never decides."""
    torch = pytest.importorskip("torch")
    lp = pytest.importorskip("transformers.generation.logits_process")
    rng = np.random.default_rng(7)
    end = 3
    checked = banned_steps = 0
    for case in range(300):
        words = [rng.integers(0, 6, int(rng.integers(1, 5))).tolist() for _ in range(int(rng.integers(1, 6)))]
        suppress = rng.integers(6, 12, 2).tolist()
        begin = rng.integers(12, 18, 2).tolist()
        n_min = int((0, 0, 1, 3, 5, 9)[case % 6])
        ptr, tok, until, max_m = ops.sequence_table(words, suppress, begin, n_min, end, vocab=V)
        table = R.table_of(ptr, tok, until)
        assert max_m == max(len(w) for w in words)
        procs = [lp.NoBadWordsLogitsProcessor(words, eos_token_id=None), lp.SuppressTokensLogitsProcessor(suppress, device="cpu"),
                 lp.SuppressTokensAtBeginLogitsProcessor(begin, 1, device="cpu")]
        if n_min:
            procs.append(lp.MinNewTokensLengthLogitsProcessor(1, n_min, end, device="cpu"))
        state = R.State()
        fed = []
        for s in range(8):
            t = 19 if s == 0 else int(rng.integers(0, 6))
            fed.append(t)
            state.record(t)
            got = R.banned(table, state.count, state.tail, V, row_min=n_min)
            scores = torch.zeros((1, V))
            ids = torch.tensor([fed])
            for p in procs:
                scores = p(ids, scores)
            want = torch.isinf(scores[0]).nonzero().reshape(-1).tolist()
            assert got == want, f"case {case} step {s}: fed {fed}, words {words}, min {n_min}"
            checked += 1
            banned_steps += bool(set(got) - set(suppress))
    assert checked == 2400 and banned_steps > 600


# ----------------------------------------------------------------------------- 2. edge cases of the definition
def test_single_tokens_and_the_longest_entry():
    assert R.banned([([7], 0)], 0, R.State().tail, V) == [7], "m = 1 needs no history at all"
    w = list(range(20, 36))                                          # m = 16: the whole tail is compared
    s = R.State(w[:15])
    assert R.banned([(w, 0)], s.count, s.tail, V) == [35]
    near = R.State([w[0] + 1] + w[1:15])
    assert R.banned([(w, 0)], near.count, near.tail, V) == [], "a near miss at the oldest position"
    for at in range(15):
        miss = list(w[:15])
        miss[at] = 1
        m = R.State(miss)
        assert R.banned([(w, 0)], m.count, m.tail, V) == []
    short = R.State(w[1:15])
    assert R.banned([(w, 0)], short.count, short.tail, V) == [], "m - 1 > count"
    assert R.banned([(w + [1], 0)], s.count, s.tail, V) == [], "an entry longer than SEQ_MAX is never active"


def test_until_boundaries_and_row_min():
    for u in (1, 2, 5):
        at, after = R.State([9] * u), R.State([9] * (u + 1))
        assert R.banned([([4], u)], at.count, at.tail, V) == [4], "count == u is still active"
        assert R.banned([([4], u)], after.count, after.tail, V) == [], "count == u + 1 is not"
    s = R.State([9, 9, 9])
    assert R.banned([([4], R.ROW)], s.count, s.tail, V, row_min=3) == [4]
    assert R.banned([([4], R.ROW)], s.count, s.tail, V, row_min=2) == []
    assert R.banned([([4], R.ROW)], s.count, s.tail, V, row_min=0) == [], "a row value of 0 is never active"
    assert R.banned([([4], R.ROW)], s.count, s.tail, V, row_min=None) == [], "no row_min: never active"
    one = R.State([9])
    assert R.banned([([4], R.ROW)], one.count, one.tail, V, row_min=0) == []
    assert R.banned([([4], -2)], s.count, s.tail, V, row_min=5) == [], "an unknown until word is never active"


def test_separators_and_tokens_outside_the_vocabulary():
    s = R.State([5, -1])
    assert s.tail[-1] == -1 and s.count == 2
    assert R.banned([([5, -1, 6], 0), ([-1, 6], 0)], s.count, s.tail, V) == [], "-1 matches nothing, not even -1"
    big = R.State([5, V + 3])
    assert R.banned([([5, V + 3, 6], 0)], big.count, big.tail, V) == [], "a history token >= V matches nothing"
    assert R.banned([([5, V + 3, 6], 0)], big.count, big.tail, V + 10) == [6]
    ok = R.State([5])
    assert R.banned([([5, V], 0), ([5, -1], 0), ([V + 1], 0)], ok.count, ok.tail, V) == [], "a last token outside [0, V) bans nothing"
    huge = R.State([1 << 31, -(1 << 40), 1 << 40])
    assert huge.tail[-3:].tolist() == [-1, -1, -1] and huge.count == 3
    off = R.State([5], count=-1)
    off.record(6)
    assert off.count == -1 and off.tail[-1] == 5 and R.banned([([6], 0)], off.count, off.tail, V) == []


def test_ban_row_and_step():
    bits = np.arange(V, dtype=np.uint16) + 0x3F00
    bits[7] = 0x7FC0
    s = R.State([5])
    out, cols = R.step(bits, s, 6, [([5, 6, 7], 0), ([6, 7], 0), ([9], 0)])
    assert cols == [7, 9] and out[7] == R.NINF and out[9] == R.NINF and s.count == 2
    rest = np.setdiff1d(np.arange(V), cols)
    assert np.array_equal(out[rest], bits[rest])


# ----------------------------------------------------------------------------- 3. the table builder and the value checks
def test_table_builder():
    ptr, tok, until, max_m = ops.sequence_table([[1, 2, 3], [4]], [5, 6], [7], 2, 9, vocab=V)
    assert ptr.dtype == np.int32 and tok.dtype == np.int32 and until.dtype == np.int32
    assert R.table_of(ptr, tok, until) == [([1, 2, 3], 0), ([4], 0), ([5], 0), ([6], 0), ([7], 1), ([9], R.ROW)] and max_m == 3
    ptr, tok, until, max_m = ops.sequence_table()
    assert ptr.tolist() == [0] and tok.size == 0 and until.size == 0 and max_m == 0
    assert R.table_of(*ops.sequence_table(min_new_tokens=0, end_token_id=9)[:3]) == []
    assert R.table_of(*ops.sequence_table(min_new_tokens=0, end_token_id=9, row_entry=True)[:3]) == [([9], R.ROW)]
    assert R.table_of(*ops.sequence_table(min_new_tokens=[0, 4], end_token_id=9)[:3]) == [([9], R.ROW)]
    assert ops.sequence_table(suppress_tokens=[3])[3] == 1
    assert (ops.SEQ_MAX, ops.SEQ_TAIL, ops.SEQ_ROW) == (R.SEQ_MAX, R.TAIL, R.ROW)


@pytest.mark.parametrize("kw", [
    dict(bad_words_ids=[[]]), dict(bad_words_ids=[1, 2]), dict(bad_words_ids="ab"), dict(bad_words_ids=[list(range(17))]),
    dict(bad_words_ids=[[1, -1]]), dict(bad_words_ids=[[1, V]]), dict(bad_words_ids=[[1.5]]), dict(bad_words_ids=[[True]]),
    dict(suppress_tokens=[V]), dict(suppress_tokens=3), dict(begin_suppress_tokens=[-2]), dict(begin_suppress_tokens="x"),
    dict(min_new_tokens=-1, end_token_id=2), dict(min_new_tokens=1.5, end_token_id=2), dict(min_new_tokens=True, end_token_id=2),
    dict(min_new_tokens=3), dict(min_new_tokens=[0, 2]), dict(min_new_tokens=2, end_token_id=V), dict(min_new_tokens=[1, 2, 3], end_token_id=2),
    dict(suppress_tokens=list(range(40)) * 103),
])
def test_check_sequences_refuses(kw):
    with pytest.raises(ValueError):
        ops.check_sequences(vocab=V, rows=2, **kw)


def test_check_sequences_accepts():
    words, suppress, begin, mins, end = ops.check_sequences([[1, 2], (3,)], np.array([4, 5]), [6.0], [0, 3], 7, vocab=V, rows=2)
    assert (words, suppress, begin, mins, end) == ([[1, 2], [3]], [4, 5], [6], [0, 3], 7)
    assert ops.check_sequences() == ([], [], [], 0, None)
    assert ops.check_sequences(min_new_tokens=0)[3] == 0, "min_new_tokens = 0 needs no end token"
    assert len(ops.check_sequences(bad_words_ids=[list(range(16))], vocab=V)[0][0]) == 16
    assert len(ops.check_sequences(suppress_tokens=list(range(V)) * 81 + list(range(46)), vocab=V)[1]) == ops.SEQ_ENTRIES_MAX
    with pytest.raises(ValueError):
        ops.check_sequences(suppress_tokens=list(range(V)) * 81 + list(range(46)), min_new_tokens=1, end_token_id=3, vocab=V)


# ----------------------------------------------------------------------------- 4. the beam walk
@pytest.mark.parametrize("K", [1, 2, 3, 10])
def test_beam_walk_equals_the_plain_history_of_the_reconstructed_sequence(K):
    """random back-pointer arrays: for every row and step the beam form's (count, tail) are the plain form's after feeding the start
    token and the row's reconstructed tokens (BeamDecodeSession.result()'s walk) - cut to the max_m - 1 tokens the walk reads"""
    rng = np.random.default_rng(K)
    B, T = 2, 24
    Rn = B * K
    tok = rng.integers(0, V, (T, Rn)).astype(np.int32)
    par = rng.integers(0, K, (T, Rn)).astype(np.int32)
    par[5] = np.tile(np.arange(K)[::-1], B)                  # a swap
    par[6] = 0                                               # all children of one parent
    starts = [11, 12]
    for t in (0, 1, 2, 5, 7, 20, T - 1):
        for r in range(Rn):
            b, beam = divmod(r, K)
            fed_now = starts[b] if t == 0 else int(tok[t - 1, r])
            seq, i = [], beam                                # the tokens of row r's beam after t steps, by result()'s walk
            for u in range(t - 1, -1, -1):
                seq.append(int(tok[u, b * K + i]))
                i = int(par[u, b * K + i])
            fed = [starts[b]] + seq[::-1]
            assert fed[-1] == fed_now
            count, tail = R.history_state(fed)
            for max_m in (1, 2, 3, 16):
                want = tail.copy()
                want[:R.TAIL - (max_m - 1)] = -1
                got_count, got_tail = R.beam_state(tok, par, t, r, K, fed_now, starts[b], max_m)
                assert got_count == count == t + 1 and np.array_equal(got_tail, want), f"t={t} r={r} max_m={max_m}"
    assert R.beam_state(tok, par, T, 0, K, 1, 11, 16)[0] == -1 and R.beam_state(tok, par, -1, 0, K, 1, 11, 16)[0] == -1
    bad = par.copy()
    bad[4] = K                                               # a parent outside the request ends the walk: the fed token alone
    _, tail = R.beam_state(tok, bad, 5, 0, K, 1, 11, 16)
    assert tail.tolist() == [-1] * (R.TAIL - 1) + [1]


# ----------------------------------------------------------------------------- 5. the keyword surface
KEYS = ("bad_words_ids", "suppress_tokens", "begin_suppress_tokens", "min_new_tokens")


def test_sessions_take_the_keywords_and_beams_do_not_exclude_them():
    from unimedvl_amd import beam, decode
    assert set(KEYS) <= set(inspect.signature(decode.DecodeSession.__init__).parameters)
    for fn in (beam.BeamDecodeSession.__init__, beam.beam_generate):
        params = inspect.signature(fn).parameters
        assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in KEYS), "explicit keywords, not **excluded"
    assert not set(KEYS) & set(beam.BEAM_EXCLUDES)
    assert "copy_sequence_state" in dir(decode.DecodeSession)
    assert "min_new_tokens" in inspect.signature(decode.DecodeSession.set_slot).parameters
