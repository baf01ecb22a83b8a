"""bad_words_ids / suppress_tokens / begin_suppress_tokens / min_new_tokens through the engine at the tiny configuration (B = 3, 24
steps, eager and graph): the session against the plain-Python definition (tests/sequence_ban_ref.py) applied on the host to the
per-step logits of a session WITHOUT the stage that is fed the same tokens through forced_ids - bit for bit, step by step -, what the
two keywords mean for the output, the slot state across rounds, set_slot and re-captures, every other control on together, the
unfused step, the batcher, beam search against tests/beam_ref.py with the reference mask in its model function, chat, the
VQAInferencer keys and the refusals.  The only tolerance is the header's 1e-4 on a log-probability."""
import functools

import numpy as np
import pytest
import torch

import beam_ref
import penalty_ref as P
import sequence_ban_ref as R
import test_beam_engine_gpu as BE
import test_ngram_engine_gpu as NE
from conftest import NEW_TOKEN_IDS
from test_logprob_gpu import model  # noqa: F401  (the tiny engine fixture)
from test_ngram_engine_gpu import BOUND, STEPS, T, _bits, _ids, _session, _stepwise

pytestmark = pytest.mark.gpu
BOS, EOS = NEW_TOKEN_IDS["bos_token_id"], NEW_TOKEN_IDS["eos_token_id"]


@pytest.fixture(autouse=True)
def pinned_split(monkeypatch):
    monkeypatch.setenv("UMV_DECODE_NSPLIT", "2")      # a request's logits do not depend on the slot or the round it is served in


@functools.lru_cache(maxsize=None)
def _plain(model):
    """the plain greedy run: (start tokens [3], picks [STEPS, 3]) as lists"""
    s = _session(model, use_graph=True)
    with torch.no_grad():
        s.step(STEPS)
    return s.in_ids[0].tolist(), s.pred_ids.cpu().numpy()


def _fed(model, r):
    start, picks = _plain(model)
    return [int(start[r])] + [int(t) for t in picks[:, r]]


def _first_bigram(fed, at):
    """the bigram fed[at], fed[at + 1] and the index of its first occurrence in fed"""
    big = [fed[at], fed[at + 1]]
    return big, next(j for j in range(len(fed) - 1) if fed[j:j + 2] == big)


def _keywords(model):
    """a table made from the plain run's own output, so that every kind of entry bans something: a bigram of every sample, a trigram
    of sample 0, sample 1's pick at step 10 suppressed, sample 2's first pick suppressed at the beginning, and minimums 0 / 5 / 9 on
    an end token that sample 1 and 2 pick early"""
    _, picks = _plain(model)
    words = [_first_bigram(_fed(model, r), 5)[0] for r in range(3)] + [_fed(model, 0)[8:11]]
    return dict(bad_words_ids=words, suppress_tokens=[int(picks[10, 1])], begin_suppress_tokens=[int(picks[0, 2])],
                min_new_tokens=[0, 5, 9], end_token_id=int(picks[1, 1]))


def _table(kw, vocab):
    from unimedvl_amd import ops
    ptr, tok, until, _ = ops.sequence_table(kw.get("bad_words_ids"), kw.get("suppress_tokens"), kw.get("begin_suppress_tokens"),
                                            kw.get("min_new_tokens", 0), kw.get("end_token_id"), vocab=vocab)
    return R.table_of(ptr, tok, until)


def _replay(model, kw, use_graph, steps=STEPS, greedy=True, forced=None, **other):
    """The replay check.  A = the session with the stage; B = the same session without it, fed A's tokens through forced_ids.  At
    every step the reference ban applied on the host to B's logits must give A's logits bit for bit; a greedy A must have picked
    their argmax (the lowest column among equals), any A a column that is not banned.  Log-probabilities, where A records them, are
    within 1e-4 of the fp64 softmax of the banned logits; the device's counts and tails are the reference's.  Returns (A, columns
    banned per step and sample)."""
    a = _session(model, steps, use_graph=use_graph, forced_ids=forced, **kw, **other)
    assert (a.graph is not None) == use_graph and a.seq_table is not None
    a_logits = _stepwise(a, steps)
    fed_next = a.pred_ids.clone() if forced is None else torch.where(forced.to(a.pred_ids.device) >= 0, forced.to(a.pred_ids.device), a.pred_ids)
    b = _session(model, steps, use_graph=False, forced_ids=fed_next, **other)
    assert b.seq_table is None
    b_logits = _stepwise(b, steps)
    assert torch.equal(a.in_ids, b.in_ids), "the plain session was fed other tokens"
    table = _table(kw, model.cfg.vocab)
    mins = kw.get("min_new_tokens", 0)
    mins = mins if isinstance(mins, list) else [mins] * 3
    states = [R.State() for _ in range(3)]
    flips, banned = [], []
    lp = a.pred_logprobs.cpu().numpy() if a.pred_logprobs is not None else None
    temp = other.get("temperature", 0.0) if other.get("do_sample") else 0.0
    for s in range(steps):
        banned.append([])
        for r, st in enumerate(states):
            want, cols = R.step(b_logits[s][r], st, int(a.in_ids[s, r]), table, mins[r])
            banned[-1].append(cols)
            got = a_logits[s][r]
            assert P.same_bits(got, want).all(), f"step {s} sample {r}: columns {np.flatnonzero(~P.same_bits(got, want))[:8]} differ"
            tok = int(a.pred_ids[s, r])
            if greedy:
                v = P.bf16_float(got).astype(np.float64)
                if tok != int(np.flatnonzero(v == v.max())[0]):
                    flips.append((s, r, tok))
            elif tok in cols:
                flips.append((s, r, tok))
            if lp is not None and (forced is None or int(forced[s, r]) < 0):
                assert abs(float(lp[s, r]) - P.logprob(got, tok, temp)) <= BOUND, f"step {s} sample {r}: log-probability"
    assert not flips, f"(step, sample, token) that are not the pick of the banned logits: {flips}"
    for r, st in enumerate(states):
        assert int(a.seq_count[r]) == st.count and a.seq_tail[r].tolist() == st.tail.tolist(), f"sample {r}: the device's history"
    return a, banned


# ----------------------------------------------------------------------------- 1. the replay check
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_replay_step_by_step(model, use_graph):
    kw = _keywords(model)
    a, banned = _replay(model, kw, use_graph)
    _, picks = _plain(model)
    assert all(any(step[r] for step in banned) for r in range(3)), "a sample never banned anything: the check is vacuous"
    assert sum(len(c) > 1 for step in banned for c in step) > 0, "no step banned two columns"
    assert not np.array_equal(a.pred_ids.cpu().numpy(), picks), "the stage changed nothing"


# ----------------------------------------------------------------------------- 2. what the keywords mean
@pytest.mark.parametrize("n", [0, 1, 6])
def test_min_new_tokens_holds_the_end_token_back(model, n):
    """the end token is the model's own pick of sample 0 at step 2: absent before index n for every sample, and a sample whose plain
    run does not pick it before index n decodes as the plain run does, token for token"""
    _, picks = _plain(model)
    end = int(picks[2, 0])
    if n == 0:
        s = _session(model, use_graph=True, min_new_tokens=0, end_token_id=end)
        assert s.seq_table is None, "min_new_tokens = 0 is off: nothing allocated"
        return
    s = _session(model, use_graph=True, min_new_tokens=n, end_token_id=end)
    with torch.no_grad():
        s.step(STEPS)
    got = s.pred_ids.cpu().numpy()
    assert end not in got[:n].flatten().tolist(), f"the end token before index {n}"
    changed = 0
    for r in range(3):
        hits = np.flatnonzero(picks[:n, r] == end)
        if hits.size == 0:
            assert np.array_equal(got[:, r], picks[:, r]), f"sample {r}: nothing was banned, yet the output moved"
        else:
            changed += 1
            assert np.array_equal(got[:hits[0], r], picks[:hits[0], r]) and got[hits[0], r] != end
    assert n < 6 or changed >= 1, "sample 0 picks the end token at step 2: a minimum of 6 must have moved it"
    assert s.seq_count.tolist() == [STEPS] * 3 and s.seq_row_min.tolist() == [n] * 3


def test_bad_words_ids_bans_the_bigram(model):
    """a bigram from the plain greedy output of sample 0: the new output is identical before it and different at it, and no sample
    is ever fed it"""
    fed = _fed(model, 0)
    big, j = _first_bigram(fed, 5)
    s = _session(model, use_graph=True, bad_words_ids=[big])
    with torch.no_grad():
        s.step(STEPS)
    new = [int(s.in_ids[0, 0])] + s.pred_ids[:, 0].tolist()
    assert new[:j + 1] == fed[:j + 1] and new[j + 1] != fed[j + 1], (big, j, new, fed)
    for r in range(3):
        seq = [int(s.in_ids[0, r])] + s.pred_ids[:, r].tolist()
        assert all(seq[i:i + 2] != big for i in range(len(seq) - 1)), f"sample {r} holds the bad word"
    assert s.seq_row_min is None


def test_suppress_and_begin_suppress(model):
    _, picks = _plain(model)
    first, later = int(picks[0, 0]), int(picks[3, 1])
    s = _session(model, use_graph=True, suppress_tokens=[later], begin_suppress_tokens=[first])
    with torch.no_grad():
        s.step(STEPS)
    got = s.pred_ids.cpu().numpy()
    assert later not in got.flatten().tolist() and first not in got[0].tolist() and got[0, 0] != picks[0, 0]


# ----------------------------------------------------------------------------- 3. slot state
def test_rewind_outputs_keeps_the_state(model):
    kw = _keywords(model)
    whole, rounds = _session(model, STEPS, use_graph=True, **kw), _session(model, STEPS, use_graph=True, **kw)
    got = []
    with torch.no_grad():
        whole.step(STEPS)
        for _ in range(STEPS // 4):
            rounds.rewind_outputs()
            rounds.step(4)
            got.append(rounds.pred_ids[:4].clone())
    assert torch.equal(torch.cat(got), whole.pred_ids)
    assert torch.equal(rounds.seq_count, whole.seq_count) and torch.equal(rounds.seq_tail, whole.seq_tail)
    assert whole.seq_count.tolist() == [STEPS] * 3 and rounds.seq_row_min.tolist() == [0, 5, 9]


def test_set_slot_starts_a_slot_over_and_leaves_the_neighbours(model):
    _, picks = _plain(model)
    half, k = STEPS // 2, 7
    kw = dict(_keywords(model), min_new_tokens=[0, 0, 0], sequence_row_min=True)
    end = kw["end_token_id"]

    def run(change):
        s = _session(model, STEPS, use_graph=True, **kw)
        graph = s.graph
        with torch.no_grad():
            s.step(half)
            if change:
                torch.cuda.synchronize()
                s.set_slot(1, int(s.ids[1]), int(s.kv_len[1]) - 1, int(s.tok_pos[1]), min_new_tokens=k)
                assert int(s.seq_count[1]) == 0 and s.seq_tail[1].tolist() == [-1] * R.TAIL and s.seq_row_min.tolist() == [0, k, 0]
            s.step(STEPS - half)
        torch.cuda.synchronize()
        assert s.graph is graph, "no re-capture"
        return s
    base, changed = run(False), run(True)
    for b in (0, 2):
        assert torch.equal(base.pred_ids[:, b], changed.pred_ids[:, b]) and torch.equal(base.seq_tail[b], changed.seq_tail[b])
    assert torch.equal(base.pred_ids[:half], changed.pred_ids[:half])
    assert base.seq_count.tolist() == [STEPS] * 3 and changed.seq_count.tolist() == [STEPS, STEPS - half, STEPS]
    assert end not in changed.pred_ids[half:half + k, 1].tolist()
    off = _session(model, 4, use_graph=False)
    off.set_slot(0, 5, 3, 3, min_new_tokens=0)
    with pytest.raises(ValueError, match="sequence_row_min"):
        off.set_slot(0, 5, 3, 3, min_new_tokens=2)
    with pytest.raises(ValueError):
        changed.set_slot(0, 5, 3, 3, min_new_tokens=-1)


def test_copy_sequence_state_carries_the_slots(model):
    kw = _keywords(model)
    a = _session(model, 8, use_graph=False, **kw)
    with torch.no_grad():
        a.step(8)
    b = _session(model, 8, use_graph=False, **dict(kw, min_new_tokens=[1, 1, 1]))
    b.copy_sequence_state(a, [0, 2])
    assert b.seq_count.tolist() == [8, 0, 8] and b.seq_row_min.tolist() == [0, 1, 9]
    assert torch.equal(b.seq_tail[0], a.seq_tail[0]) and torch.equal(b.seq_tail[2], a.seq_tail[2]) and b.seq_tail[1].tolist() == [-1] * R.TAIL
    plain = _session(model, 8, use_graph=False)
    plain.copy_sequence_state(a)
    b.copy_sequence_state(plain)
    assert b.seq_count.tolist() == [8, 0, 8]


# ----------------------------------------------------------------------------- 4. with everything else on
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_replay_with_every_other_control_on(model, use_graph):
    from unimedvl_amd.constraints import TokenAutomaton
    kw = _keywords(model)
    allowed = TokenAutomaton.from_allowed_tokens(sorted(set(range(0, 300, 2)) | {BOS, kw["end_token_id"]}))
    other = dict(do_sample=True, temperature=T, seed=77, top_p=0.9, logprobs=True, top_logprobs=2, constraint=allowed, repetition_penalty=1.2,
                 presence_penalty=0.5, logit_bias={17: 1.5}, no_repeat_ngram_size=2)
    a, banned = _replay(model, kw, use_graph, greedy=False, **other)
    assert a.step_end == "truncated" and a.pen is not None and a.con_state is not None and a.ng_hist is not None
    assert sum(bool(c) for step in banned for c in step) >= 15, "the begin entry and the two minimums ban at 3 + 5 + 9 steps"
    assert all(int(t) % 2 == 0 or int(t) == kw["end_token_id"] for t in a.pred_ids.flatten().tolist()), "the constraint still holds"


def test_replay_with_forced_tokens(model):
    """forced_ids feed the two tokens of a bad word and the end token inside a minimum: a forced token is recorded and fed, banned
    or not, and the first token of the word bans its second at the step it is fed"""
    kw = _keywords(model)
    word = kw["bad_words_ids"][0]
    forced = torch.full((STEPS, 3), -1, dtype=torch.int64)
    forced[4, 0], forced[5, 0], forced[2, 2] = word[0], word[1], kw["end_token_id"]
    a, banned = _replay(model, kw, True, forced=forced, logprobs=True)
    assert word[1] in banned[5][0] and int(a.in_ids[6, 0]) == word[1] and int(a.in_ids[3, 2]) == kw["end_token_id"]
    assert kw["end_token_id"] in banned[2][2] and float(a.pred_logprobs[5, 0]) == float("-inf")


def test_replay_with_row_sampling(model):
    from unimedvl_amd.sampling import SamplingParams
    rows = [SamplingParams(), SamplingParams(do_sample=True, temperature=T, top_p=0.9, seed=5), SamplingParams(do_sample=True, temperature=1.3, seed=6)]
    a, banned = _replay(model, _keywords(model), True, greedy=False, row_sampling=rows)
    assert a.step_end == "rows" and sum(bool(c) for step in banned for c in step) >= 6


def test_the_unfused_step_gives_the_fused_steps_tokens(model, monkeypatch):
    kw = _keywords(model)
    with torch.no_grad():
        fused = _session(model, 12, use_graph=True, **kw)
        fused.step(12)
        with monkeypatch.context() as mp:
            mp.setenv("UMV_DECODE_FUSED_ARGMAX", "0")
            plain = _session(model, 12, use_graph=True, **kw)
        assert fused.fused_argmax and not plain.fused_argmax and plain.seq_table is not None
        plain.step(12)
    assert torch.equal(fused.pred_ids, plain.pred_ids) and torch.equal(fused.logits.view(torch.int16), plain.logits.view(torch.int16))
    assert torch.equal(fused.seq_tail, plain.seq_tail)


# ----------------------------------------------------------------------------- 5. the batcher
MINS = [None, 0, 6, 3, None, 9, 1]


def _serve(model, order, check_every, table, paged=False, max_context=256, budget=20, long_at=None, min_default=2):
    """the requests of test_ngram_engine_gpu with the minimums MINS (None: the batcher's default) and a logit bias that makes the end
    token every request's pick wherever it is not banned - so an answer holds exactly its minimum of tokens"""
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.serving import ContinuousBatcher
    reqs = NE._requests(long_at)
    srv = ContinuousBatcher(model, ToyTokenizer(NEW_TOKEN_IDS), NEW_TOKEN_IDS, lambda x: x, slots=3, max_context=max_context,
                            max_new_tokens=budget, check_every=check_every, paged=paged, min_new_tokens=min_default,
                            logit_bias={EOS: 60.0}, **table)
    rids = {i: srv.submit(*reqs[i], min_new_tokens=MINS[i]) for i in order}
    got = srv.run()
    return {i: _ids(got[r]) for i, r in rids.items()}, srv


@functools.lru_cache(maxsize=None)
def _batcher_table(model):
    """a batcher-wide table from the answers without one: a bigram of request 5's answer as a string (bad_words), request 2's third
    token suppressed, request 3's first token suppressed at the beginning"""
    free, _ = _serve(model, range(7), 4, {})
    assert [len(free[i]) for i in range(7)] == [2 if n is None else n for n in MINS]
    return dict(bad_words=[f"{free[5][2]} {free[5][3]}"], suppress_tokens=[free[2][2]], begin_suppress_tokens=[free[3][0]]), free


def test_batcher_per_request_minimums_next_to_a_table(model):
    """7 requests on 3 slots: a request's tokens depend on neither the admission order, the round length nor the cache kind, and
    equal the request served alone; every request holds exactly its minimum of tokens (the end token is biased to win wherever it
    is not banned), no bad word, no suppressed token"""
    table, free = _batcher_table(model)
    base, srv = _serve(model, range(7), 4, table)
    assert srv._min_on and srv.banned["bad_words_ids"] == [[int(v) for v in table["bad_words"][0].split()]]
    for what, (other, _) in (("reversed, check_every 16", _serve(model, reversed(range(7)), 16, table)),
                             ("paged, reversed", _serve(model, reversed(range(7)), 4, table, paged=True))):
        for i in range(7):
            assert other[i] == base[i], f"{what}: request {i} answers {other[i]}, not {base[i]}"
    for i in range(7):
        alone, _ = _serve(model, [i], 4, table)
        assert alone[i] == base[i], f"request {i} served alone: {alone[i]} against {base[i]}"
        n = 2 if MINS[i] is None else MINS[i]
        big = srv.banned["bad_words_ids"][0]
        assert len(base[i]) == n, f"request {i}: {len(base[i])} tokens, minimum {n}"
        assert all(base[i][j:j + 2] != big for j in range(len(base[i]) - 1)) and table["suppress_tokens"][0] not in base[i]
        assert not base[i] or base[i][0] != table["begin_suppress_tokens"][0]
    assert all(base[i] != free[i] for i in (2, 3, 5)), "the table changed nothing for the requests it was made from"


def test_batcher_recapture_carries_the_state(model):
    """a 280-token prompt admitted in the second wave outgrows a cache reserved for 16 tokens of context while the other slots are in
    the middle of their requests: the step is re-captured, counts, tails and minimums carried over, and every answer is the one of
    the run that reserved enough up front"""
    table, _ = _batcher_table(model)
    order = [1, 3, 5, 2, 0, 4, 6]
    want, big = _serve(model, order, 4, table, max_context=1024, long_at=2)
    got, small = _serve(model, order, 4, table, max_context=16, long_at=2)
    assert big.stats["cache_grows"] == 0 and small.stats["cache_grows"] > 0
    assert got == want and [len(got[i]) for i in range(7)] == [2 if n is None else n for n in MINS]


# ----------------------------------------------------------------------------- 6. beams
def _beam_kw(model):
    """a bad bigram from the unbanned search's best hypothesis of request 0, its second token suppressed at the beginning for
    nobody else, and a minimum of 4 on the end token"""
    res, _, _, _ = BE._searched(model, False)
    eos = BE._end_token(model)
    best, other = res[0][0]["tokens"], res[1][0]["tokens"]
    assert len(best) >= 3
    return dict(bad_words_ids=[best[1:3]], suppress_tokens=[next(int(t) for t in other[1:] if t != eos)],
                begin_suppress_tokens=[int(other[0])], min_new_tokens=[4, 6])


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_the_search_is_beam_ref_over_the_plain_engine_with_the_reference_mask(model, use_graph):
    """beam_ref driven by the plain engine (eager forced sessions over K copies of a request's prompt) with the reference's banned
    columns set to -inf in its model function; no hypothesis is shorter than min_new_tokens + 1, none holds a bad word or a
    suppressed token"""
    from unimedvl_amd.decode import DecodeSession
    K, STEPS_B, B = BE.K, BE.STEPS, BE.B
    eos = BE._end_token(model)
    kw = _beam_kw(model)
    cache, gi, sess = BE._beam(model, end_token_id=eos, num_return_sequences=K, use_graph=use_graph, eos_check_every=4, **kw)
    assert sess.seq_table is not None and sess.seq_tail is None and sess.seq_row_min.tolist() == [4] * K + [6] * K
    with torch.no_grad():
        res = sess.run().result()
    nsplit = sess.nsplit
    sess.release()
    table = _table(dict(kw, end_token_id=eos), model.cfg.vocab)
    starts = gi["packed_start_tokens"].tolist()
    banned_any = [0]

    def engine(b):
        def fn(prefixes):
            cache, gi = BE._ctx(model, [BE.PROMPTS[b]] * K, paged=False)
            n = len(prefixes[0])
            forced = torch.full((n + 1, K), -1, dtype=torch.int64)
            if n:
                forced[:n] = torch.tensor(prefixes).t()
            with torch.no_grad():
                s = DecodeSession(model.language_model, cache, gi["packed_start_tokens"], gi["packed_query_position_ids"], n + 1,
                                  forced_ids=forced, use_graph=False, nsplit=nsplit)
                s.step(n + 1)
            logits = s.logits.float().cpu()
            for i, prefix in enumerate(prefixes):
                count, tail = R.history_state([starts[b]] + list(prefix))
                cols = R.banned(table, count, tail, model.cfg.vocab, kw["min_new_tokens"][b])
                banned_any[0] += bool(cols)
                logits[i, cols] = float("-inf")
            return torch.log_softmax(logits, -1).numpy()
        return fn
    for b in range(B):
        want = beam_ref.search(engine(b), K, STEPS_B, eos, length_penalty=1.0, early_stopping=False).hypotheses()
        assert [h["tokens"] for h in res[b]] == [h["tokens"] for h in want]
        for g, w in zip(res[b], want):
            assert abs(g["total"] - w["total"]) <= BOUND * len(g["tokens"]) and abs(g["score"] - w["score"]) <= BOUND
        for h in res[b]:
            toks = h["tokens"]
            assert len(toks) >= kw["min_new_tokens"][b] + 1, f"request {b}: a hypothesis of {len(toks)} tokens"
            assert all(toks[i:i + 2] != kw["bad_words_ids"][0] for i in range(len(toks) - 1)) and kw["suppress_tokens"][0] not in toks
            assert toks[0] != kw["begin_suppress_tokens"][0]
    assert banned_any[0] > 0
    plain, _, _, _ = BE._searched(model, False)
    assert [h["tokens"] for h in res[0]] != [h["tokens"] for h in plain[0]], "the stage changed nothing for request 0"


def test_generate_text_with_beams_takes_the_keywords(model):
    eos = BE._end_token(model)
    kw = _beam_kw(model)
    cache, gi = BE._ctx(model)
    with torch.no_grad():
        ids = model.generate_text(past_key_values=cache, max_length=BE.STEPS, end_token_id=eos, num_beams=BE.K, **kw, **gi)
    for b in range(BE.B):
        toks = model.last_beam_hypotheses[b][0]["tokens"]
        assert ids[1:len(toks) + 1, b].tolist() == toks and len(toks) >= kw["min_new_tokens"][b] + 1
    for bad in (dict(no_repeat_ngram_size=2), dict(repetition_penalty=1.3)):
        with pytest.raises(ValueError):
            model.generate_text(past_key_values=cache, max_length=4, num_beams=3, bad_words_ids=[[5, 6]], **bad, **gi)


# ----------------------------------------------------------------------------- 7. chat and the inferencer keys
def test_chat_and_the_inferencer_keys(model):
    from PIL import Image
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.interactive_vqa_inferencer import VQAInferencer
    from unimedvl_amd.transforms import ImageTransform
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    ident = lambda x: x   # noqa: E731
    free = _ids(model.chat(tok, NEW_TOKEN_IDS, ident, [], "5 17 40 23", max_length=20))
    assert len(free) >= 3
    word = f"{free[1]} {free[2]}"
    banned = _ids(model.chat(tok, NEW_TOKEN_IDS, ident, [], "5 17 40 23", max_length=20, bad_words=[word]))
    j = next(i for i in range(len(free) - 1) if free[i:i + 2] == free[1:3])
    assert banned[:j + 1] == free[:j + 1] and banned[j + 1:j + 2] != free[j + 1:j + 2]
    assert all(banned[i:i + 2] != free[1:3] for i in range(len(banned) - 1))
    by_ids = _ids(model.chat(tok, NEW_TOKEN_IDS, ident, [], "5 17 40 23", max_length=20, bad_words_ids=[free[1:3]]))
    assert by_ids == banned
    n = len(free) + 4
    longer, ids, lps = model.chat(tok, NEW_TOKEN_IDS, ident, [], "5 17 40 23", max_length=n + 6, min_new_tokens=n, return_logprobs=True,
                                  suppress_tokens=[free[0]])
    assert len(ids) >= n and free[0] not in ids and all(np.isfinite(lps))
    beams = model.chat(tok, NEW_TOKEN_IDS, ident, [], "5 17 40 23", max_length=10, num_beams=3, min_new_tokens=6, begin_suppress_tokens=[free[0]])
    best = model.last_beam_hypotheses[0][0]["tokens"]
    assert len(best) >= 7 and best[0] != free[0] and beams == "".join(f" {t}" for t in model.last_beam_hypotheses[0][0]["tokens_no_end"])
    pil = Image.fromarray(np.random.default_rng(3).integers(0, 255, (60, 84, 3), dtype=np.uint8))

    def make(**cfg):
        v = VQAInferencer(dict({"max_new_tokens": 12, "do_sample": False}, **cfg))
        v.load_model(model=model, tokenizer=tok, new_token_ids=NEW_TOKEN_IDS)
        v.image_transform = ImageTransform(56, 28, 14)
        return v
    a = _ids(make().infer_single(pil, "5 6 7 8")["answer"])
    assert len(a) >= 2
    b = _ids(make(bad_words=[f"{a[0]} {a[1]}"], min_new_tokens=12).infer_single(pil, "5 6 7 8")["answer"])
    assert b[0] == a[0] and b[1] != a[1]
    c = _ids(make(suppress_tokens=[a[0]], begin_suppress_tokens=[a[1]], bad_words_ids=[[1, 2]]).infer_single(pil, "5 6 7 8")["answer"])
    assert a[0] not in c and c[0] != a[1]


# ----------------------------------------------------------------------------- 8. refusals
def test_refusals(model):
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.serving import ContinuousBatcher
    V = model.cfg.vocab
    for bad in (dict(min_new_tokens=3), dict(min_new_tokens=[1, 2], end_token_id=5), dict(min_new_tokens=-1, end_token_id=5),
                dict(min_new_tokens=2, end_token_id=V), dict(bad_words_ids=[[]]), dict(bad_words_ids=[5, 6]), dict(bad_words_ids=[list(range(17))]),
                dict(bad_words_ids=[[V]]), dict(suppress_tokens=[-1]), dict(suppress_tokens=5), dict(begin_suppress_tokens=[1.5]),
                dict(sequence_row_min=True)):
        with pytest.raises(ValueError):
            _session(model, 4, use_graph=False, **bad)
    off = _session(model, 4, use_graph=False, bad_words_ids=[], suppress_tokens=[], min_new_tokens=0, end_token_id=V + 5)
    assert off.seq_table is None and off.seq_tail is None and off.seq_count is None, "off: nothing is allocated"
    cache, gi = BE._ctx(model, paged=False)
    for kw in (dict(bad_words_ids=[[5, 6]]), dict(min_new_tokens=2, end_token_id=EOS), dict(suppress_tokens=[5])):
        with pytest.raises(ValueError, match="draft_len"):
            model.generate_text(past_key_values=cache, max_length=4, draft_len=2, **kw, **gi)
    with pytest.raises(ValueError, match="end_token_id"):
        model.generate_text(past_key_values=cache, max_length=4, min_new_tokens=2, **gi)
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    with pytest.raises(ValueError):
        model.chat(tok, NEW_TOKEN_IDS, lambda x: x, [], "5 17", max_length=4, bad_words="5 6")
    with pytest.raises(ValueError):
        ContinuousBatcher(model, tok, NEW_TOKEN_IDS, lambda x: x, slots=1, min_new_tokens=[1])
    srv = ContinuousBatcher(model, tok, NEW_TOKEN_IDS, lambda x: x, slots=1)
    with pytest.raises(ValueError):
        srv.submit([], "5 6", min_new_tokens=-2)
