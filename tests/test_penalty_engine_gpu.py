"""Logit penalties through the engine at the tiny configuration: DecodeSession against the numpy model of the definition
(tests/penalty_ref.py) applied to the raw logits of an unpenalised session that is fed the same tokens, graph replay against the
un-captured step, the sampled + truncated step against a host loop over the stand-alone entries, a banned token, neutral keywords, the
batcher's history reset, and the unfused step.  Everything is exact: ids equal, logits and log-probabilities bit for bit."""
import numpy as np
import pytest
import torch

import penalty_ref as P
from conftest import NEW_TOKEN_IDS

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
T = 0.7
PROMPTS = [[11, 22, 33, 44, 55], [66, 77, 88], [99, 111, 122, 133]]
BIAS = {17: 1.5, 44: -2.0}
PEN = dict(repetition_penalty=1.2, presence_penalty=0.5, frequency_penalty=0.25, logit_bias=BIAS)
REF = dict(r=1.2, presence=0.5, frequency=0.25)
CONTEXT = [p + [NEW_TOKEN_IDS["bos_token_id"]] for p in PROMPTS]


@pytest.fixture(scope="module")
def model(tiny_weights):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.config import UniMedVLConfig
    cfg, sd, _, _ = tiny_weights
    return Bagel(UniMedVLConfig.from_dict(cfg), lambda n: sd[n], device="cuda", visual_gen=False)


def _session(model, steps=8, B=3, **kw):
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


N_STATIC = max(len(set(c)) for c in CONTEXT) + len(BIAS)      # the session's layout: room for the longest context, then the biased columns


def _histories(V, steps, context=CONTEXT, bias=BIAS):
    return [P.History(V, cap=N_STATIC + steps, context=c, bias=bias, n_static=N_STATIC) for c in context]


def test_teacher_check_against_the_model(model):
    """A decodes with penalties; B, without, is fed A's tokens through forced_ids.  At every step B's raw logits pushed through the
    model with A's history are A's logits bit for bit, and A's token is that row's argmax (lowest column among equals)."""
    steps, V = 10, model.cfg.vocab
    with torch.no_grad():
        a = _session(model, steps, use_graph=False, penalty_context_ids=CONTEXT, **PEN)
        a_logits = []
        for s in range(steps):
            a.step(1)
            a_logits.append(a.logits.clone())
        b = _session(model, steps, use_graph=False, forced_ids=a.pred_ids.clone())
        hists = _histories(V, steps)
        changed = 0
        for s in range(steps):
            b.step(1)
            raw = _bits(b.logits)
            for r, h in enumerate(hists):
                h.record(int(a.in_ids[s, r]))
                want = P.adjust_row(raw[r], h, **REF)
                got = _bits(a_logits[s][r])
                assert P.same_bits(got, want).all(), f"step {s} row {r}: columns {np.flatnonzero(~P.same_bits(got, want))[:8]}"
                changed += int((want != raw[r]).sum())
                v = P.bf16_float(got).astype(np.float64)
                assert int(a.pred_ids[s, r]) == int(np.flatnonzero(v == v.max())[0]), f"step {s} row {r}: not the argmax of the adjusted row"
    assert changed > steps * 3, "the penalties must have changed logits"
    assert torch.equal(a.in_ids[1:], a.pred_ids[:-1])
    # the device's history is the model's
    assert a.pen_static == N_STATIC and a.pen_list.shape[1] == N_STATIC + steps
    for r, h in enumerate(hists):
        assert int(a.pen_len[r]) == h.len
        assert np.array_equal(a.pen_count[r].cpu().numpy().view(np.uint32), h.count)
        assert a.pen_list[r].tolist() == h.list.tolist()


@pytest.mark.parametrize("mode", ["greedy", "sample", "truncated"])
def test_graph_replay_equals_the_uncaptured_step(model, mode):
    kw = dict(greedy={}, sample=dict(do_sample=True, temperature=T, seed=77),
              truncated=dict(do_sample=True, temperature=T, seed=77, top_k=20, top_p=0.9))[mode]
    with torch.no_grad():
        g = _session(model, 8, use_graph=True, logprobs=True, penalty_context_ids=CONTEXT, **PEN, **kw)
        assert g.graph is not None and g.pen is not None
        g.step(8)
        e = _session(model, 8, use_graph=False, logprobs=True, penalty_context_ids=CONTEXT, **PEN, **kw)
        e.step(8)
    assert torch.equal(g.pred_ids, e.pred_ids) and torch.equal(g.in_ids, e.in_ids)
    assert torch.equal(g.logits.view(torch.int16), e.logits.view(torch.int16))
    assert torch.equal(g.pred_logprobs.view(torch.int32), e.pred_logprobs.view(torch.int32))
    assert torch.equal(g.pen_count, e.pen_count) and torch.equal(g.pen_len, e.pen_len)
    plain = _session(model, 8, use_graph=True, **kw)
    plain.step(8)
    assert not torch.equal(plain.pred_ids, g.pred_ids), "the penalties changed nothing"


def test_sampled_truncated_session_equals_a_host_loop_over_the_stand_alone_entries(model):
    """tokens of a captured session with do_sample + top_k + penalties = per step: the stand-alone penalty kernel on an unpenalised
    session's raw logits (no partials), then umv_sample_truncated_bf16 with the session's (seed, step)"""
    from unimedvl_amd import ops
    steps, V, seed, top_k = 8, model.cfg.vocab, 77, 12
    with torch.no_grad():
        s = _session(model, steps, use_graph=True, do_sample=True, temperature=T, seed=seed, top_k=top_k, penalty_context_ids=CONTEXT, **PEN)
        s.step(steps)
        b = _session(model, steps, use_graph=False)
        hists = _histories(V, steps)
        count = torch.from_numpy(np.stack([h.count for h in hists]).view(np.int32)).cuda()
        vlist = torch.from_numpy(np.stack([h.list for h in hists])).cuda()
        bias = torch.from_numpy(np.stack([h.bias for h in hists])).cuda()
        length = torch.full((3,), -1, dtype=torch.int32, device="cuda")
        for i in range(steps):
            fed = b.ids.clone()
            b.step(1)
            logits = b.logits.clone()
            ops.logit_penalty(logits, fed, count, vlist, length, N_STATIC, bias=bias, temperature=T, **PEN_OPS)
            tok = ops.sample_truncated(logits, T, seed, step=torch.tensor([i], dtype=torch.int64, device="cuda"), top_k=top_k)
            assert torch.equal(tok, s.pred_ids[i]), f"step {i}: host loop {tok.tolist()} session {s.pred_ids[i].tolist()}"
            b.ids.copy_(tok)            # the next step embeds the host loop's token


PEN_OPS = dict(repetition_penalty=1.2, presence_penalty=0.5, frequency_penalty=0.25)


def test_a_banned_token_never_appears(model):
    steps = 64
    with torch.no_grad():
        free = _session(model, steps, use_graph=True)
        free.step(steps)
        seen = free.pred_ids.flatten().tolist()
        banned = max(set(seen), key=seen.count)              # the unpenalised run's most frequent token
        s = _session(model, steps, use_graph=True, logit_bias={banned: float("-inf")})
        s.step(steps)
    assert banned in seen and banned not in s.pred_ids.flatten().tolist()
    assert (s.logits[:, banned] == float("-inf")).all()


def test_neutral_keywords_are_todays_step(model, monkeypatch):
    from unimedvl_amd import ops
    calls = {}

    def record(name):
        log = calls.setdefault(name, [])
        seen = []
        for fn in [n for n in dir(ops) if callable(getattr(ops, n)) and not n.startswith("_") and n[0].islower()]:
            orig = getattr(ops, fn)
            if getattr(orig, "__module__", None) != ops.__name__ or isinstance(orig, type):
                continue

            def wrap(*a, _orig=orig, _fn=fn, **k):
                log.append(_fn)
                return _orig(*a, **k)
            seen.append((fn, orig))
            monkeypatch.setattr(ops, fn, wrap)
        return seen
    with torch.no_grad():
        record("old")
        old = _session(model, 8, use_graph=False)
        old.step(2)
        monkeypatch.undo()
        record("new")
        new = _session(model, 8, use_graph=False, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0,
                       logit_bias={5: 0.0}, penalty_context_ids=CONTEXT)
        new.step(2)
        monkeypatch.undo()
        old.step(6)
        new.step(6)
    assert calls["old"] == calls["new"] and "logit_penalty" not in calls["new"] and "gemm" in calls["new"]
    assert new.pen is None and new.pen_count is None and new.pen_list is None and new.pen_len is None and new.pen_bias is None
    assert torch.equal(old.pred_ids, new.pred_ids) and torch.equal(old.logits.view(torch.int16), new.logits.view(torch.int16))
    with torch.no_grad():
        on = _session(model, 8, use_graph=False, repetition_penalty=1.2)
        record("on")
        on.step(1)
        monkeypatch.undo()
    assert calls["on"].count("logit_penalty") == 1 and calls["on"].index("logit_penalty") == calls["on"].index("decode_step_end_argmax") - 1


def test_batcher_resets_the_history_and_keeps_it_across_rounds(model):
    """one slot, greedy: the same request twice with another in between gives the same tokens both times - the history was reset at
    admission - and they are generate_text's (through chat) with the same penalties - it survived the rounds (check_every = 4 < budget)"""
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.serving import ContinuousBatcher
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    ident = lambda x: x   # noqa: E731
    reqs = [([], "5 17 40 23"), ([], "200 31 7"), ([], "5 17 40 23")]
    pen = dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25, logit_bias={9: 2.0})
    for prompt_too in (False, True):
        srv = ContinuousBatcher(model, tok, NEW_TOKEN_IDS, ident, slots=1, max_context=256, max_new_tokens=14, check_every=4,
                                penalize_prompt=prompt_too, **pen)
        rids = [srv.submit(images, prompt) for images, prompt in reqs]
        got = srv.run()
        assert got[rids[0]] == got[rids[2]]
        for rid, (images, prompt) in zip(rids, reqs):
            assert got[rid] == model.chat(tok, NEW_TOKEN_IDS, ident, images, prompt, max_length=15, penalize_prompt=prompt_too, **pen), rid
    plain = ContinuousBatcher(model, tok, NEW_TOKEN_IDS, ident, slots=1, max_context=256, max_new_tokens=14, check_every=4)
    rid = plain.submit(*reqs[0])
    assert plain.run()[rid] != got[rids[0]], "the penalties changed nothing"


def test_batcher_reserves_room_for_the_longest_prompt_only(model, monkeypatch):
    """penalize_prompt: the session's static section is sized by the prompts admitted so far (a power of two, at least 32), never by the
    vocabulary; a longer prompt re-captures the step with more room and the running request of the other slot keeps its history - the
    answers are chat's, request by request."""
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd import decode
    from unimedvl_amd.serving import ContinuousBatcher
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    ident = lambda x: x   # noqa: E731
    long_prompt = " ".join(str(5 + i) for i in range(40))                 # 40 distinct tokens: more than the first reservation of 32
    reqs = [([], "5 17 40 23", 14), ([], "200 31 7", 3), ([], long_prompt, 6), ([], "9 8", 5)]
    pen = dict(repetition_penalty=1.3, presence_penalty=0.5, logit_bias={9: 2.0})
    rooms = []
    real = decode.DecodeSession._init_penalties

    def spy(self, *args, **kw):
        real(self, *args, **kw)
        rooms.append((self.pen_room, self.pen_static))
    monkeypatch.setattr(decode.DecodeSession, "_init_penalties", spy)
    srv = ContinuousBatcher(model, tok, NEW_TOKEN_IDS, ident, slots=2, max_context=256, max_new_tokens=14, check_every=4,
                            penalize_prompt=True, **pen)
    rids = [srv.submit(images, prompt, max_new_tokens=n) for images, prompt, n in reqs]
    got = srv.run()
    monkeypatch.undo()
    assert rooms == [(32, 33), (64, 65)], rooms              # one re-capture, when the 40-token prompt arrived; 1 biased column
    for rid, (images, prompt, n) in zip(rids, reqs):
        assert got[rid] == model.chat(tok, NEW_TOKEN_IDS, ident, images, prompt, max_length=n + 1, penalize_prompt=True, **pen), rid


def test_vqa_inferencer_config_keys_and_overrides(model):
    from PIL import Image
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.interactive_vqa_inferencer import VQAInferencer
    from unimedvl_amd.transforms import ImageTransform
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    pil = Image.fromarray(np.random.default_rng(3).integers(0, 255, (60, 84, 3), dtype=np.uint8))

    def make(**cfg):
        v = VQAInferencer(dict({"max_new_tokens": 10, "do_sample": False}, **cfg))
        v.load_model(model=model, tokenizer=tok, new_token_ids=NEW_TOKEN_IDS)
        v.image_transform = ImageTransform(56, 28, 14)
        return v
    plain, pen = make(), make(repetition_penalty=1.3, presence_penalty=0.5, penalize_prompt=True)
    a = plain.infer_single(pil, "5 6 7 8")["answer"]
    b = pen.infer_single(pil, "5 6 7 8")["answer"]
    assert a != b, "the config keys changed nothing"
    assert plain.infer_single(pil, "5 6 7 8", repetition_penalty=1.3, presence_penalty=0.5, penalize_prompt=True)["answer"] == b
    assert pen.infer_single(pil, "5 6 7 8", repetition_penalty=1.0, presence_penalty=0.0, penalize_prompt=False)["answer"] == a
    first = int(a.split()[0])
    assert str(first) not in plain.infer_single(pil, "5 6 7 8", logit_bias={first: float("-inf")})["answer"].split()
    with pytest.raises(ValueError, match="repetition_penalty"):
        plain.infer_single(pil, "5 6 7 8", repetition_penalty=0.0)


def test_the_unfused_step_gives_the_fused_steps_ids(model, monkeypatch):
    """(DecodeSession reads UMV_DECODE_FUSED_ARGMAX when it is constructed, so the variable is set around the constructor)"""
    with torch.no_grad():
        fused = _session(model, 8, use_graph=True, penalty_context_ids=CONTEXT, **PEN)
        fused.step(8)
        with monkeypatch.context() as mp:
            mp.setenv("UMV_DECODE_FUSED_ARGMAX", "0")
            plain = _session(model, 8, use_graph=True, penalty_context_ids=CONTEXT, **PEN)
        assert fused.fused_argmax and not plain.fused_argmax and plain.pen is not None
        plain.step(8)
    assert torch.equal(fused.pred_ids, plain.pred_ids) and torch.equal(fused.logits.view(torch.int16), plain.logits.view(torch.int16))


def test_refusals(model):
    for bad in (dict(repetition_penalty=0.0), dict(presence_penalty=float("inf")), dict(logit_bias={model.cfg.vocab: 1.0}),
                dict(repetition_penalty=1.2, penalty_context_ids=[[1]]), dict(repetition_penalty=1.2, penalty_context_ids=[[-1], [], []])):
        with pytest.raises(ValueError):
            _session(model, 4, use_graph=False, **bad)
    s = _session(model, 4, use_graph=False, repetition_penalty=1.2, penalty_context_ids=[[1, 2], [], []])
    with pytest.raises(ValueError, match="room"):
        s.set_slot(0, 5, 3, 3, penalty_context_ids=[1, 2, 3])
    s.set_slot(0, 5, 3, 3, penalty_context_ids=[7])
    assert int(s.pen_len[0]) == -1 and int(s.pen_list[0, 0]) == 7 and int(s.pen_count[0].ne(0).sum()) == 1
