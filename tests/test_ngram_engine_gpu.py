"""no_repeat_ngram_size through the engine at the tiny configuration (B = 3, 24 steps, eager and graph): the n-gram session against the
plain-Python definition (tests/ngram_ref.py) applied on the host to the per-step logits of a session WITHOUT the ban that is fed the
same tokens through forced_ids - bit for bit, step by step -, the slot state across rounds, set_slot and re-captures, every other
sampler control on together, per-row sizes, the batcher with per-request sizes, and chat.  The only tolerance is the header's 1e-4 on
a log-probability."""
import numpy as np
import pytest
import torch

import ngram_ref as R
import penalty_ref as P
from conftest import NEW_TOKEN_IDS

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
T = 0.7
STEPS = 24
BOS = NEW_TOKEN_IDS["bos_token_id"]
PROMPTS = [[11, 22, 33, 44, 55], [66, 77, 88], [99, 111, 122, 133]]
BOUND = 1e-4          # of a log-probability (include/unimedvl_hip.h, token log-probabilities)
NINF = 0xFF80


@pytest.fixture(scope="module")
def model(tiny_weights):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.config import UniMedVLConfig
    cfg, sd, _, _ = tiny_weights
    return Bagel(UniMedVLConfig.from_dict(cfg), lambda n: sd[n], device="cuda", visual_gen=False)


@pytest.fixture(autouse=True)
def pinned_split(monkeypatch):
    monkeypatch.setenv("UMV_DECODE_NSPLIT", "2")      # a request's logits do not depend on the slot or the round it is served in


def _session(model, steps=STEPS, B=3, **kw):
    from unimedvl_amd.decode import DecodeSession
    from unimedvl_amd.kvcache import NaiveCache

    class Tok:
        def encode(self, s):
            return PROMPTS[int(s) % 3]
    cache = NaiveCache(model.cfg.layers)
    gi, kvl, rope = model.prepare_prompts([0] * B, [0] * B, [str(i) for i in range(B)], Tok(), NEW_TOKEN_IDS)
    cache = model.forward_cache_update_text(cache, **gi)
    gi = model.prepare_start_tokens(kvl, rope, NEW_TOKEN_IDS)
    with torch.no_grad():
        return DecodeSession(model.language_model, cache, gi["packed_start_tokens"], gi["packed_query_position_ids"], steps, **kw)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _stepwise(sess, steps):
    """run `steps` steps one by one: the logits every step left"""
    logits = []
    with torch.no_grad():
        for _ in range(steps):
            sess.step(1)
            logits.append(_bits(sess.logits))
    torch.cuda.synchronize()
    return logits


def _replay(model, sizes, use_graph, contexts=None, steps=STEPS, greedy=True, **other):
    """The replay check.  A = the n-gram session; B = the same session without the ban, fed A's tokens through forced_ids.  At every
    step the reference ban applied on the host to B's logits must give A's logits bit for bit; a greedy A must have emitted their
    argmax (the lowest column among equals), any A a column that is not banned - anything else counts as a flip, and none is allowed.
    Log-probabilities, where A records them, are within 1e-4 of the fp64 softmax of the banned logits.  Returns (A, columns banned
    per step and sample)."""
    B = 3
    contexts = contexts or [[] for _ in range(B)]
    per_row = sizes if isinstance(sizes, (list, tuple)) else [sizes] * B
    a = _session(model, steps, use_graph=use_graph, no_repeat_ngram_size=sizes, ngram_context_ids=contexts, **other)
    assert (a.graph is not None) == use_graph and a.ng_hist is not None
    a_logits = _stepwise(a, steps)
    b = _session(model, steps, use_graph=False, forced_ids=a.pred_ids.clone(), **other)
    assert b.ng_hist is None
    b_logits = _stepwise(b, steps)
    assert torch.equal(a.in_ids, b.in_ids), "the plain session was fed other tokens"
    hists = [R.History(a.ng_hist.shape[1], c) for c in contexts]
    flips, banned = [], []
    lp = a.pred_logprobs.cpu().numpy() if a.pred_logprobs is not None else None
    for s in range(steps):
        banned.append([])
        for r, h in enumerate(hists):
            want, cols = R.step(b_logits[s][r], h, int(a.in_ids[s, r]), per_row[r])
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
            if lp is not None:
                assert abs(float(lp[s, r]) - P.logprob(got, tok, other.get("temperature", 0.0) if other.get("do_sample") else 0.0)) <= BOUND, f"step {s} sample {r}: log-probability"
    assert not flips, f"(step, sample, token) that are not the pick of the banned logits: {flips}"
    for r, h in enumerate(hists):
        assert int(a.ng_len[r]) == h.len and a.ng_hist[r].tolist() == h.hist.tolist(), f"sample {r}: the device's history"
    return a, banned


# ----------------------------------------------------------------------------- 1. the replay check
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_replay_step_by_step(model, use_graph):
    a, banned = _replay(model, 3, use_graph)
    assert sum(bool(c) for step in banned for c in step) > 0, "n = 3 never banned anything: the check is vacuous"
    plain = _session(model, use_graph=True)
    plain.step(STEPS)
    assert not torch.equal(plain.pred_ids, a.pred_ids), "the ban changed nothing"


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_n1_emits_no_token_twice(model, use_graph):
    """n = 1: every step bans the whole history - the arm that is not vacuous by construction"""
    a, banned = _replay(model, 1, use_graph)
    assert all(len(c) >= min(s + 1, 2) for s, step in enumerate(banned) for c in step)
    for r in range(3):
        fed = a.in_ids[:, r].tolist() + [int(a.pred_ids[-1, r])]
        assert len(set(fed)) == STEPS + 1, f"sample {r} was fed a token twice: {fed}"


@pytest.mark.parametrize("n", [2, 3])
def test_a_seeded_context_bans_at_the_first_step(model, n):
    """ngram_context_ids = [x, bos, y, bos, z] (n = 2; with a filler in front of every bos at n = 3) and start token bos: the first
    step already bans y and z - here the plain session's best two tokens, so the ban moves the first pick"""
    plain = _session(model, 1, use_graph=False)
    plain.step(1)
    top2 = plain.logits.float().topk(2, dim=-1).indices.tolist()
    w = 7
    if n == 2:
        contexts = [[5, BOS, y, BOS, z] for y, z in top2]
    else:
        contexts = [[5, w, BOS, y, w, BOS, z, w] for y, z in top2]
    a, banned = _replay(model, n, True, contexts=contexts, steps=6)
    for r, (y, z) in enumerate(top2):
        assert {y, z} <= set(banned[0][r]), f"sample {r}: the first step banned {banned[0][r]}, not {y} and {z}"
        assert int(a.pred_ids[0, r]) not in (y, z) and int(plain.pred_ids[0, r]) == y


# ----------------------------------------------------------------------------- 2. slot state
def test_rewind_outputs_keeps_the_history(model):
    whole = _session(model, STEPS, use_graph=True, no_repeat_ngram_size=2)
    rounds = _session(model, STEPS, use_graph=True, no_repeat_ngram_size=2)      # (the cache holds STEPS tokens; the outputs rewind)
    got = []
    with torch.no_grad():
        whole.step(STEPS)
        for _ in range(STEPS // 4):
            rounds.rewind_outputs()
            rounds.step(4)
            got.append(rounds.pred_ids[:4].clone())
    assert torch.equal(torch.cat(got), whole.pred_ids)
    assert torch.equal(rounds.ng_len, whole.ng_len) and torch.equal(rounds.ng_hist, whole.ng_hist)
    assert whole.ng_len.tolist() == [STEPS] * 3 and int(rounds.step_idx[0]) == 4
    plain = _session(model, STEPS, use_graph=True)
    plain.step(STEPS)
    assert not torch.equal(plain.pred_ids, whole.pred_ids), "n = 2 changed nothing"


def test_set_slot_starts_a_history_over_and_leaves_the_neighbours(model):
    half = STEPS // 2

    def run(change):
        s = _session(model, STEPS, use_graph=True, no_repeat_ngram_size=1, ngram_context_ids=[[1, 2], [3], []], ngram_context_room=4)
        graph = s.graph
        with torch.no_grad():
            s.step(half)
            if change:
                torch.cuda.synchronize()
                s.set_slot(1, int(s.ids[1]), int(s.kv_len[1]) - 1, int(s.tok_pos[1]), ngram_context_ids=[9, 8, 7])
                assert int(s.ng_len[1]) == 3 and s.ng_hist[1, :3].tolist() == [9, 8, 7]
            s.step(STEPS - half)
        torch.cuda.synchronize()
        assert s.graph is graph, "no re-capture"
        return s
    base, changed = run(False), run(True)
    for b in (0, 2):
        assert torch.equal(base.pred_ids[:, b], changed.pred_ids[:, b]) and torch.equal(base.ng_hist[b], changed.ng_hist[b])
    assert torch.equal(base.pred_ids[:half], changed.pred_ids[:half])
    assert base.ng_len.tolist() == [2 + STEPS, 1 + STEPS, STEPS] and changed.ng_len.tolist() == [2 + STEPS, 3 + STEPS - half, STEPS]
    # slot 1 forgot its first half: it may emit those tokens again, and n = 1 still holds inside the second half
    second = changed.in_ids[half:, 1].tolist() + [int(changed.pred_ids[-1, 1])]
    assert len(set(second)) == len(second) and not {9, 8, 7} & set(changed.pred_ids[half:, 1].tolist())
    with pytest.raises(ValueError, match="ngram_context_room"):
        changed.set_slot(1, 5, 3, 3, ngram_context_ids=[1, 2, 3, 4, 5])


def test_copy_ngram_history_carries_the_slots_into_a_larger_session(model):
    a = _session(model, 8, use_graph=False, no_repeat_ngram_size=[2, 0, 3], ngram_context_ids=[[4, 5], [], [6]])
    with torch.no_grad():
        a.step(8)
    b = _session(model, 8, use_graph=False, no_repeat_ngram_size=[1, 1, 1], ngram_context_room=16, ngram_history=32)
    before = (b.ng_hist.clone(), b.ng_len.clone(), b.ng_row_n.clone())
    b.copy_ngram_history(a, [0, 2])
    for r in (0, 2):
        n = int(a.ng_len[r])
        assert int(b.ng_len[r]) == n and b.ng_hist[r, :n].tolist() == a.ng_hist[r, :n].tolist() and int(b.ng_row_n[r]) == int(a.ng_row_n[r])
    assert torch.equal(b.ng_hist[1], before[0][1]) and int(b.ng_len[1]) == int(before[1][1]) and int(b.ng_row_n[1]) == 1
    with pytest.raises(ValueError, match="layout"):
        a.copy_ngram_history(b)


# ----------------------------------------------------------------------------- 3. with everything else on
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_replay_with_every_other_control_on(model, use_graph):
    from unimedvl_amd.constraints import TokenAutomaton
    allowed = TokenAutomaton.from_allowed_tokens(list(range(0, 300, 2)) + [BOS])
    other = dict(do_sample=True, temperature=T, seed=77, top_p=0.9, logprobs=True, constraint=allowed, repetition_penalty=1.2,
                 presence_penalty=0.5, logit_bias={17: 1.5})
    a, banned = _replay(model, [1, 2, 1], use_graph, greedy=False, **other)
    assert a.step_end == "truncated" and a.pen is not None and a.con_state is not None
    assert all(step[0] and step[2] for step in banned), "n = 1 bans at every step"
    assert all(int(t) % 2 == 0 for t in a.pred_ids.flatten().tolist()), "the constraint still holds"


def test_the_unfused_step_gives_the_fused_steps_tokens(model, monkeypatch):
    with torch.no_grad():
        fused = _session(model, 8, use_graph=True, no_repeat_ngram_size=1)
        fused.step(8)
        with monkeypatch.context() as mp:
            mp.setenv("UMV_DECODE_FUSED_ARGMAX", "0")
            plain = _session(model, 8, use_graph=True, no_repeat_ngram_size=1)
        assert fused.fused_argmax and not plain.fused_argmax and plain.ng_hist is not None
        plain.step(8)
    assert torch.equal(fused.pred_ids, plain.pred_ids) and torch.equal(fused.logits.view(torch.int16), plain.logits.view(torch.int16))


# ----------------------------------------------------------------------------- 4. per-row sizes
def test_per_row_sizes(model):
    from unimedvl_amd.sampling import SamplingParams
    plain = _session(model, use_graph=True)
    plain_logits = _stepwise(plain, STEPS)
    a, banned = _replay(model, [0, 1, 3], True)
    assert torch.equal(a.pred_ids[:, 0], plain.pred_ids[:, 0]) and not any(step[0] for step in banned)
    a2 = _session(model, use_graph=True, no_repeat_ngram_size=[0, 1, 3])
    a2_logits = _stepwise(a2, STEPS)
    assert all(np.array_equal(x[0], y[0]) for x, y in zip(a2_logits, plain_logits)), "sample 0's logits are the plain session's"
    rows = _session(model, use_graph=True, row_sampling=[SamplingParams(no_repeat_ngram_size=n) for n in (0, 1, 3)])
    with torch.no_grad():
        rows.step(STEPS)
    assert rows.ng_row_n.tolist() == [0, 1, 3] and torch.equal(rows.pred_ids, a.pred_ids) and torch.equal(rows.ng_hist, a.ng_hist)
    off = _session(model, 4, use_graph=False, row_sampling=[SamplingParams()] * 3)
    assert off.ng_hist is None and off.ng_row_n is None
    with pytest.raises(ValueError, match="ngram_history"):
        off.set_slot(0, 5, 3, 3, sampling=SamplingParams(no_repeat_ngram_size=2))
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        _session(model, 4, use_graph=False, row_sampling=[SamplingParams()] * 3, no_repeat_ngram_size=2)
    reserved = _session(model, 4, use_graph=False, row_sampling=[SamplingParams()] * 3, ngram_history=8)
    reserved.set_slot(0, 5, 3, 3, sampling=SamplingParams(no_repeat_ngram_size=2))
    assert reserved.ng_row_n.tolist() == [2, 0, 0]


# ----------------------------------------------------------------------------- 5. the batcher, per request
SIZES = [0, 1, 3, 1, 0, 3, 1]


def _requests(long_at=None):
    """seven requests, every other one with an image; long_at: that request's prompt is 280 tokens long instead of 4"""
    g = torch.Generator().manual_seed(21)
    reqs = [([torch.randn(3, 42, 56, generator=g).clamp(-1, 1)] if i % 2 == 0 else [], f"{5 + i} {17 + 3 * i} {40 + i} {17 + 3 * i}")
            for i in range(7)]
    if long_at is not None:
        reqs[long_at] = (reqs[long_at][0], " ".join(str(int(v)) for v in torch.randint(5, 290, (280,), generator=g)))
    return reqs


def _serve(model, order, check_every, paged=False, max_context=256, budget=20, long_at=None, **kw):
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.sampling import SamplingParams
    from unimedvl_amd.serving import ContinuousBatcher
    reqs = _requests(long_at)
    srv = ContinuousBatcher(model, ToyTokenizer(NEW_TOKEN_IDS), NEW_TOKEN_IDS, lambda x: x, slots=3, max_context=max_context,
                            max_new_tokens=budget, check_every=check_every, per_request_sampling=True, seed=9, paged=paged, **kw)
    rids = {i: srv.submit(*reqs[i], sampling=SamplingParams(no_repeat_ngram_size=SIZES[i])) for i in order}
    got = srv.run()
    return {i: _ids(got[r]) for i, r in rids.items()}, srv


def _ids(answer):
    """the token ids behind an answer of the toy tokenizer (the two image markers render as words)"""
    for name, t in (("<|vision_start|>", NEW_TOKEN_IDS["start_of_image"]), ("<|vision_end|>", NEW_TOKEN_IDS["end_of_image"])):
        answer = answer.replace(name, f" {t}")
    return [int(t) for t in answer.split()]


def test_batcher_per_request_sizes(model):
    """7 requests on 3 slots with sizes 0 / 1 / 3 mixed: a request's tokens depend on neither the admission order, the round length nor
    the cache kind; an n = 1 request repeats nothing; the slot an n = 1 request leaves serves its next request as if admitted first"""
    base, srv = _serve(model, range(7), 4)
    assert srv._ng_on and srv.stats["cache_grows"] == 0
    for what, (other, _) in (("reversed, check_every 16", _serve(model, reversed(range(7)), 16)),
                             ("paged, check_every 16", _serve(model, range(7), 16, paged=True)),
                             ("paged, reversed", _serve(model, reversed(range(7)), 4, paged=True))):
        for i in range(7):
            assert other[i] == base[i], f"{what}: request {i} answers {other[i]}, not {base[i]}"
    for i, n in enumerate(SIZES):
        if n == 1:
            assert len(set(base[i])) == len(base[i]) and BOS not in base[i], f"request {i} (n = 1) repeats a token: {base[i]}"
    assert any(len(base[i]) >= 8 for i in range(7))
    # slot 0 serves request 0, then - in admission order - a later one: every request admitted behind an n = 1 request equals itself alone
    for i in (3, 4, 5, 6):
        alone, _ = _serve(model, [i], 4)
        assert alone[i] == base[i], f"request {i} served alone: {alone[i]} against {base[i]}"
    plain, _ = _serve(model, [1], 4)
    from oracle.toy_tokenizer import ToyTokenizer
    free = model.chat(ToyTokenizer(NEW_TOKEN_IDS), NEW_TOKEN_IDS, lambda x: x, *_requests()[1], max_length=21)
    assert _ids(free) != plain[1], "n = 1 changed nothing for request 1"


def test_batcher_recapture_carries_the_histories(model, monkeypatch):
    """a 280-token prompt admitted in the second wave outgrows a cache reserved for 16 tokens of context while the other slots are in
    the middle of their requests (cache_grows > 0): the step is re-captured, the live histories carried over, and every answer is
    the one of the run that reserved enough up front; the same with the prompt as history, where the long prompt also outgrows the
    history's context room"""
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd import decode
    order = [1, 3, 5, 2, 0, 4, 6]
    seeded = []
    real = decode.DecodeSession._reset_ngram_slot

    def spy(self, b, context):
        seeded.append(tuple(context))
        real(self, b, context)
    monkeypatch.setattr(decode.DecodeSession, "_reset_ngram_slot", spy)
    prompts = {tuple(ToyTokenizer(NEW_TOKEN_IDS).encode(prompt)) for _, prompt in _requests(2)}
    for kw in (dict(), dict(no_repeat_ngram_prompt=True)):
        want, big = _serve(model, order, 4, max_context=1024, long_at=2, **kw)
        del seeded[:]
        got, small = _serve(model, order, 4, max_context=16, long_at=2, **kw)
        assert big.stats["cache_grows"] == 0 and small.stats["cache_grows"] > 0
        assert got == want
        assert (small._ng_room >= 280) == bool(kw) and small._ng_hist >= 20
        # what the slots' histories were seeded with: nothing, or - every request at its admission - exactly its prompt's tokens
        assert set(seeded) - {()} == (prompts if kw else set()), sorted(set(seeded) - {()})


def test_batcher_wide_size_and_chat(model):
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.serving import ContinuousBatcher
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    ident = lambda x: x   # noqa: E731
    reqs = [([], "5 17 40 23"), ([], "200 31 7"), ([], "5 17 40 23")]
    for prompt_too in (False, True):
        srv = ContinuousBatcher(model, tok, NEW_TOKEN_IDS, ident, slots=1, max_context=256, max_new_tokens=14, check_every=4,
                                no_repeat_ngram_size=1, no_repeat_ngram_prompt=prompt_too)
        rids = [srv.submit(images, prompt) for images, prompt in reqs]
        got = srv.run()
        assert got[rids[0]] == got[rids[2]]
        for rid, (images, prompt) in zip(rids, reqs):
            want = model.chat(tok, NEW_TOKEN_IDS, ident, images, prompt, max_length=15, no_repeat_ngram_size=1, no_repeat_ngram_prompt=prompt_too)
            assert got[rid] == want, rid
            ids = _ids(want)
            assert len(set(ids)) == len(ids), f"chat(no_repeat_ngram_size=1) repeats a token id: {ids}"
            if prompt_too:
                assert not set(ids) & set(tok.encode(prompt)), "a prompt token was emitted"
    answer, ids, lps = model.chat(tok, NEW_TOKEN_IDS, ident, [], "5 17 40 23", max_length=20, no_repeat_ngram_size=1, return_logprobs=True)
    assert len(ids) >= 2 and len(set(ids)) == len(ids) and all(np.isfinite(lps))
    free = model.chat(tok, NEW_TOKEN_IDS, ident, [], "5 17 40 23", max_length=20)
    assert free != answer


def test_vqa_inferencer_config_key(model):
    from PIL import Image
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.interactive_vqa_inferencer import VQAInferencer
    from unimedvl_amd.transforms import ImageTransform
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    pil = Image.fromarray(np.random.default_rng(3).integers(0, 255, (60, 84, 3), dtype=np.uint8))

    def make(**cfg):
        v = VQAInferencer(dict({"max_new_tokens": 12, "do_sample": False}, **cfg))
        v.load_model(model=model, tokenizer=tok, new_token_ids=NEW_TOKEN_IDS)
        v.image_transform = ImageTransform(56, 28, 14)
        return v
    a = make().infer_single(pil, "5 6 7 8")["answer"]
    b = make(no_repeat_ngram_size=1, no_repeat_ngram_prompt=True).infer_single(pil, "5 6 7 8")["answer"]
    ids = _ids(b)
    assert a != b and len(set(ids)) == len(ids) and not {5, 6, 7, 8} & set(ids)


def test_refusals(model):
    for bad in (dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=17), dict(no_repeat_ngram_size=1.5), dict(no_repeat_ngram_size=True),
                dict(no_repeat_ngram_size=[1, 2]), dict(no_repeat_ngram_size=2, ngram_context_ids=[[1]]),
                dict(no_repeat_ngram_size=2, ngram_context_ids=[[1 << 31], [], []])):
        with pytest.raises(ValueError):
            _session(model, 4, use_graph=False, **bad)
    off = _session(model, 4, use_graph=False, no_repeat_ngram_size=0, ngram_context_ids=[[1], [2], [3]])
    assert off.ng_hist is None and off.ng_len is None and off.ng_row_n is None, "off: nothing is allocated"
    off.set_slot(0, 5, 3, 3, ngram_context_ids=[1, 2])       # (ignored, as penalty_context_ids is without penalties)
