"""Constrained decoding through the engine at the tiny configuration: DecodeSession(constraint=) against a plain session that is fed
the same tokens (every constrained pick is the argmax over the host-walked allowed set of the plain session's raw logits, the free
sample is untouched bit for bit), graph replay against the un-captured step, set_slot / rewind_outputs, per-row sampling with top_p
(log-probabilities against the fp64 restricted log-softmax), the convenience layers, and the batcher with a re-capture in mid-run."""
import numpy as np
import pytest
import torch

import constraint_ref as C
import penalty_ref as P
from conftest import NEW_TOKEN_IDS

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
T = 0.7
BOUND = 1e-4          # of a log-probability (include/unimedvl_hip.h, token log-probabilities; tests/logprob_ref.py)
MARGIN = 0.25         # the project's near-tie clause (tests/test_engine_gpu.py): ids are exact wherever the top-2 margin exceeds it
EOS = NEW_TOKEN_IDS["eos_token_id"]
PROMPTS = [[11, 22, 33, 44, 55], [66, 77, 88], [99, 111, 122, 133]]
CHOICES = [[10, 11, 12], [10, 11], [10, 13, 14], [20, 21]]           # a shared prefix (10), and [10, 11] is a prefix of [10, 11, 12]
SET = [40, 41, 42, 43, 44, 45, 50, 60, 70, 80, 90, 100]


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


def _choices():
    from unimedvl_amd.constraints import TokenAutomaton
    return TokenAutomaton.from_choices(CHOICES, EOS)


def _both():
    """the choice trie and the token set in one table: (automaton, {name: start state})"""
    from unimedvl_amd.constraints import TokenAutomaton
    return TokenAutomaton.union({"choices": _choices(), "set": TokenAutomaton.from_allowed_tokens(SET)})


def _emitted(column):
    """the tokens of one sample up to its first EOS (excluded), and whether EOS came"""
    out = []
    for t in column:
        if t == EOS:
            return out, True
        out.append(int(t))
    return out, False


def _same_cache(a, b, seg, n):
    for l in range(len(a.cache.slabs)):
        assert torch.equal(a.cache.slabs[l].k[seg, :, :n].view(torch.int16), b.cache.slabs[l].k[seg, :, :n].view(torch.int16)), f"layer {l}: K"
        assert torch.equal(a.cache.slabs[l].vt[seg, :, :, :n].view(torch.int16), b.cache.slabs[l].vt[seg, :, :, :n].view(torch.int16)), f"layer {l}: V^T"


# ----------------------------------------------------------------------------- greedy with choices
def test_greedy_choices_against_a_forced_plain_session(model):
    steps, V = 7, model.cfg.vocab
    auto = _choices()
    with torch.no_grad():
        a = _session(model, steps, use_graph=False, constraint=auto, constraint_states=[0, 0, -1])
        a_logits, a_states = [], [a.con_state.cpu().tolist()]
        for s in range(steps):
            a.step(1)
            a_logits.append(a.logits.clone())
            a_states.append(a.con_state.cpu().tolist())
        forced = a.pred_ids.clone()
        forced[:, 2] = -1                                  # the free sample runs free in the plain session too
        b = _session(model, steps, use_graph=False, forced_ids=forced)
        b_logits = []
        for s in range(steps):
            b.step(1)
            b_logits.append(b.logits.clone())
    pred = a.pred_ids.cpu()
    near = 0
    for r in (0, 1):
        toks, ended = _emitted(pred[:, r].tolist())
        assert ended and toks in CHOICES, f"sample {r} emitted {pred[:, r].tolist()}"
        assert (pred[len(toks):, r] == EOS).all(), "after the end token only the end token (the final state's self-loop)"
        state = 0
        for s in range(steps):
            assert a_states[s][r] == state, f"sample {r} step {s}: the device's state word against walk"
            A = auto.allowed(state).tolist()
            raw = _bits(b_logits[s][r])
            pick, best = int(pred[s, r]), C.restricted_argmax(raw, A)
            assert pick in A
            assert np.array_equal(_bits(a_logits[s][r]), C.mask_row(raw, C.Automaton(auto.row_ptr, auto.edge_token, auto.edge_next), state)), \
                f"sample {r} step {s}: the stored logits are not the plain session's, masked"
            if pick != best:
                v = P.bf16_float(raw)
                assert float(v[best]) - float(v[pick]) <= MARGIN, f"sample {r} step {s}: picked {pick}, the allowed argmax is {best}"
                near += 1
            state = auto.walk(state, [pick])
        assert a_states[steps][r] == state == auto.n_states - 1
    print(f"constrained picks that needed the {MARGIN}-logit near-tie clause: {near} of {2 * steps}")
    # the free sample: tokens, logits and cache are the plain session's, bit for bit
    assert all(st[2] == -1 for st in a_states)
    assert torch.equal(a.pred_ids[:, 2], b.pred_ids[:, 2]) and torch.equal(a.in_ids[:, 2], b.in_ids[:, 2])
    for s in range(steps):
        assert torch.equal(a_logits[s][2].view(torch.int16), b_logits[s][2].view(torch.int16)), f"step {s}: the free sample's logits"
    _same_cache(a, b, 2, a.lens0[2] + steps)


def test_all_states_free_is_the_unconstrained_session(model):
    steps = 6
    with torch.no_grad():
        a = _session(model, steps, use_graph=True, logprobs=True, constraint=_choices(), constraint_states=[-1, -1, -1])
        b = _session(model, steps, use_graph=True, logprobs=True)
        a.step(steps)
        b.step(steps)
    assert a.con_state is not None and b.con_state is None and b.con_dev is None and b.constraint is None
    assert torch.equal(a.pred_ids, b.pred_ids) and torch.equal(a.in_ids, b.in_ids)
    assert torch.equal(a.logits.view(torch.int16), b.logits.view(torch.int16))
    assert torch.equal(a.pred_logprobs.view(torch.int32), b.pred_logprobs.view(torch.int32))
    assert a.con_state.cpu().tolist() == [-1, -1, -1]
    for seg in range(3):
        _same_cache(a, b, seg, a.lens0[seg] + steps)


@pytest.mark.parametrize("mode", ["greedy", "sample", "truncated"])
def test_graph_replay_equals_the_uncaptured_step(model, mode):
    kw = dict(greedy={}, sample=dict(do_sample=True, temperature=T, seed=77),
              truncated=dict(do_sample=True, temperature=T, seed=77, top_k=20, top_p=0.9))[mode]
    auto, start = _both()
    states = [start["choices"], start["set"], -1]
    with torch.no_grad():
        g = _session(model, 8, use_graph=True, logprobs=True, constraint=auto, constraint_states=states, **kw)
        assert g.graph is not None and g.con_state.cpu().tolist() == states, "capture must leave the state words where they started"
        g.step(8)
        e = _session(model, 8, use_graph=False, logprobs=True, constraint=auto, constraint_states=states, **kw)
        e.step(8)
    assert torch.equal(g.pred_ids, e.pred_ids) and torch.equal(g.in_ids, e.in_ids)
    assert torch.equal(g.logits.view(torch.int16), e.logits.view(torch.int16))
    assert torch.equal(g.pred_logprobs.view(torch.int32), e.pred_logprobs.view(torch.int32))
    assert torch.equal(g.con_state, e.con_state)
    pred = g.pred_ids.cpu()
    toks, ended = _emitted(pred[:, 0].tolist())
    assert ended and toks in CHOICES
    assert set(pred[:, 1].tolist()) <= set(SET)
    assert g.con_state.cpu().tolist() == [auto.walk(states[r], pred[:, r].tolist()) for r in range(3)]


def test_launch_sequence(model, monkeypatch):
    """without a constraint neither kernel is launched and nothing is allocated; with one, the mask sits right in front of the step end
    (behind the penalty kernel) and the advance is the step's last launch"""
    from unimedvl_amd import ops
    log = []
    for fn in [n for n in dir(ops) if callable(getattr(ops, n)) and not n.startswith("_") and n[0].islower()]:
        orig = getattr(ops, fn)
        if getattr(orig, "__module__", None) != ops.__name__ or isinstance(orig, type):
            continue

        def wrap(*a, _orig=orig, _fn=fn, **k):
            log.append(_fn)
            return _orig(*a, **k)
        monkeypatch.setattr(ops, fn, wrap)
    with torch.no_grad():
        off = _session(model, 4, use_graph=False, constraint=None)
        del log[:]
        off.step(1)
        plain = list(log)
        on = _session(model, 4, use_graph=False, constraint=_choices(), repetition_penalty=1.2, top_logprobs=3)
        del log[:]
        on.step(1)
    monkeypatch.undo()
    assert "logit_constrain" not in plain and "constraint_advance" not in plain and off.con_state is None
    tail = ["gemm", "logit_penalty", "logit_constrain", "decode_step_end_logprob", "decode_top_logprobs", "constraint_advance"]
    assert [n for n in log if n in tail][-6:] == tail and log[-1] == "constraint_advance", log[-8:]
    assert log.count("logit_constrain") == 1 and log.count("constraint_advance") == 1
    assert [n for n in log if n not in ("logit_penalty", "logit_constrain", "decode_top_logprobs", "constraint_advance")][:-1] == plain[:-1], \
        "the rest of the step is the plain step's"


# ----------------------------------------------------------------------------- slots and rounds
def test_set_slot_repoints_a_slot_without_a_recapture(model):
    auto, start = _both()
    with torch.no_grad():
        s = _session(model, 10, use_graph=True, constraint=auto, constraint_states=[start["choices"], start["choices"], -1])
        g = s.graph
        s.step(1)
        before = s.con_state.cpu().tolist()
        s.set_slot(0, int(s.ids[0]), int(s.tok_slot[0]), int(s.tok_pos[0]))                                     # no keyword: the word stays
        assert s.con_state.cpu().tolist() == before
        s.set_slot(1, int(s.ids[1]), int(s.tok_slot[1]), int(s.tok_pos[1]), constraint_state=start["set"])
        s.set_slot(2, int(s.ids[2]), int(s.tok_slot[2]), int(s.tok_pos[2]), constraint_state=start["choices"])
        assert s.con_state.cpu().tolist() == [before[0], start["set"], start["choices"]]
        s.step(6)
    assert s.graph is g
    pred = s.pred_ids[:7].cpu()
    toks, ended = _emitted(pred[:, 0].tolist())
    assert ended and toks in CHOICES
    assert set(pred[1:, 1].tolist()) <= set(SET), "slot 1 decodes under the token set from the replay after set_slot on"
    toks, ended = _emitted(pred[1:, 2].tolist())
    assert ended and toks in CHOICES, "slot 2, free before, emits a choice from the replay after set_slot on"
    with pytest.raises(ValueError):
        s.set_slot(0, 5, 3, 3, constraint_state=auto.n_states)
    with pytest.raises(ValueError):
        _session(model, 4, use_graph=False).set_slot(0, 5, 3, 3, constraint_state=0)


def test_rewind_outputs_keeps_the_state(model):
    auto = _choices()
    with torch.no_grad():
        s = _session(model, 4, use_graph=True, constraint=auto)
        s.step(1)
        first = s.pred_ids[:1].cpu()
        word = s.con_state.cpu().tolist()
        s.rewind_outputs()
        assert s.con_state.cpu().tolist() == word == [auto.walk(0, [int(t)]) for t in first[0]]
        s.step(4)
    pred = torch.cat([first, s.pred_ids[:4].cpu()], 0)
    for r in range(3):
        toks, ended = _emitted(pred[:, r].tolist())
        assert ended and toks in CHOICES, f"sample {r}: {pred[:, r].tolist()} - the choice did not go on across the rewind"


def test_forced_foreign_token_leaves_the_automaton(model):
    from unimedvl_amd.constraints import LEFT
    auto = _choices()
    forced = torch.full((5, 3), -1, dtype=torch.int64)
    forced[1, 0] = 299                                      # no edge anywhere
    with torch.no_grad():
        s = _session(model, 5, use_graph=True, constraint=auto, forced_ids=forced)
        s.step(5)
    assert s.con_state.cpu().tolist()[0] == LEFT and int(s.in_ids[2, 0]) == 299
    assert int(s.pred_ids[0, 0]) in (10, 20) and int(s.pred_ids[1, 0]) in auto.allowed(auto.walk(0, [int(s.pred_ids[0, 0])])).tolist()
    for r in (1, 2):
        toks, ended = _emitted(s.pred_ids[:, r].tolist())
        assert ended and toks in CHOICES


def test_the_unfused_step_gives_the_fused_steps_ids(model, monkeypatch):
    auto, start = _both()
    states = [start["choices"], start["set"], -1]
    with torch.no_grad():
        fused = _session(model, 8, use_graph=True, constraint=auto, constraint_states=states)
        fused.step(8)
        with monkeypatch.context() as mp:
            mp.setenv("UMV_DECODE_FUSED_ARGMAX", "0")
            plain = _session(model, 8, use_graph=True, constraint=auto, constraint_states=states)
        assert fused.fused_argmax and not plain.fused_argmax and plain.con_state is not None
        plain.step(8)
    assert torch.equal(fused.pred_ids, plain.pred_ids) and torch.equal(fused.logits.view(torch.int16), plain.logits.view(torch.int16))
    assert torch.equal(fused.con_state, plain.con_state)


# ----------------------------------------------------------------------------- samplers
def test_row_sampling_with_top_p_stays_in_the_set_and_renormalises(model):
    from unimedvl_amd.constraints import TokenAutomaton
    from unimedvl_amd.sampling import SamplingParams
    steps = 8
    auto = TokenAutomaton.from_allowed_tokens(SET)
    params = [SamplingParams(do_sample=True, temperature=T, top_p=0.9, seed=5), SamplingParams(),
              SamplingParams(do_sample=True, temperature=1.3, top_p=0.7, top_k=6, seed=6)]
    with torch.no_grad():
        s = _session(model, steps, use_graph=True, logprobs=True, row_sampling=params, constraint=auto)
        s.step(steps)
        b = _session(model, steps, use_graph=False, forced_ids=s.pred_ids.clone())
        raw = []
        for i in range(steps):
            b.step(1)
            raw.append(_bits(b.logits))
    pred, lp = s.pred_ids.cpu(), s.pred_logprobs.cpu().double()
    assert set(pred.flatten().tolist()) <= set(SET)
    worst = 0.0
    for i in range(steps):
        for r, p in enumerate(params):
            temp = p.temperature if p.do_sample else 0.0
            worst = max(worst, abs(float(lp[i, r]) - C.restricted_logprob(raw[i][r], SET, int(pred[i, r]), temp)))
    print(f"pred_logprobs off the fp64 restricted log-softmax of the forced replay by at most {worst:.3g}")
    assert worst <= BOUND


def test_scalar_sampling_with_penalties_and_top_logprobs(model):
    from unimedvl_amd.constraints import TokenAutomaton
    steps, n = 8, 5
    auto = TokenAutomaton.from_allowed_tokens(SET[:4])
    with torch.no_grad():
        s = _session(model, steps, use_graph=True, do_sample=True, temperature=T, seed=9, top_k=3, repetition_penalty=1.3,
                     presence_penalty=0.5, top_logprobs=n, constraint=auto)
        s.step(steps)
    assert set(s.pred_ids.flatten().tolist()) <= set(SET[:4])
    top_ids, top_lp, rank = s.pred_top_ids.cpu(), s.pred_top_logprobs.cpu(), s.pred_rank.cpu()
    assert (rank >= 1).all() and (rank <= 4).all()
    assert set(top_ids[:, :, :4].flatten().tolist()) == set(SET[:4]), "the four best alternatives are the allowed tokens"
    assert torch.isfinite(top_lp[:, :, :4]).all() and (top_lp[:, :, 4] == float("-inf")).all(), "the fifth alternative is a masked column"
    assert float((torch.exp(top_lp[:, :, :4].double()).sum(-1) - 1).abs().max()) < 1e-3, "the allowed tokens' probabilities sum to one"


# ----------------------------------------------------------------------------- the convenience layers
def test_chat_choices_and_the_inferencers_key(model):
    from PIL import Image
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.interactive_vqa_inferencer import VQAInferencer
    from unimedvl_amd.transforms import ImageTransform
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    ident = lambda x: x   # noqa: E731
    texts = ["10 11 12", "10 11", "10 13 14", "20 21"]
    free = model.chat(tok, NEW_TOKEN_IDS, ident, [], "5 17 40 23", max_length=8).strip()
    assert free not in texts, "the unconstrained answer is already a choice: the test shows nothing"
    assert model.chat(tok, NEW_TOKEN_IDS, ident, [], "5 17 40 23", max_length=8, choices=texts).strip() in texts
    assert model.chat(tok, NEW_TOKEN_IDS, ident, [], "5 17 40 23", max_length=8, choices=CHOICES).strip() in texts          # token-id lists
    got = {model.chat(tok, NEW_TOKEN_IDS, ident, [], f"{5 + i} 17 40", max_length=8, choices=texts, do_sample=True, temperature=1.5).strip()
           for i in range(6)}
    assert got <= set(texts)
    answer, ids, lps = model.chat(tok, NEW_TOKEN_IDS, ident, [], "5 17 40 23", max_length=8, choices=texts, return_logprobs=True)
    assert answer.strip() in texts and ids[-1] != EOS and len(lps) == len(ids) and all(v <= 0 for v in lps)
    opened = model.chat(tok, NEW_TOKEN_IDS, ident, [], "5 17 40 23", max_length=8, choices=["10 13 14", "20 21"], choices_after="free").strip()
    assert opened.startswith("10 13 14") or opened.startswith("20 21")
    with pytest.raises(ValueError, match="constraint"):
        model.chat(tok, NEW_TOKEN_IDS, ident, [], "5 17 40 23", max_length=8, choices=texts, draft_len=2)
    with pytest.raises(ValueError):
        model.chat(tok, NEW_TOKEN_IDS, ident, [], "5 17 40 23", max_length=8, choices=["10 11", "10 11"])
    pil = Image.fromarray(np.random.default_rng(3).integers(0, 255, (60, 84, 3), dtype=np.uint8))

    def make(**cfg):
        v = VQAInferencer(dict({"max_new_tokens": 8, "do_sample": False}, **cfg))
        v.load_model(model=model, tokenizer=tok, new_token_ids=NEW_TOKEN_IDS)
        v.image_transform = ImageTransform(56, 28, 14)
        return v
    plain, guided = make(), make(choices=texts)
    assert guided.infer_single(pil, "5 6 7 8")["answer"].strip() in texts
    assert plain.infer_single(pil, "5 6 7 8", choices=["20 21", "30"])["answer"].strip() in ("20 21", "30")
    assert guided.infer_single(pil, "5 6 7 8", choices=["30 31"])["answer"].strip() == "30 31"            # the call's list wins
    assert plain.infer_single(pil, "5 6 7 8")["answer"].strip() not in texts


def test_drafts_refuse_a_constraint(model):
    from unimedvl_amd.kvcache import NaiveCache
    from unimedvl_amd.speculative import SpeculativeDecodeSession
    with pytest.raises(ValueError, match="constraint"):
        SpeculativeDecodeSession(model.language_model, NaiveCache(model.cfg.layers), None, None, 8, 2, constraint=_choices())
    with pytest.raises(ValueError, match="constraint"):
        model.generate_text(NaiveCache(model.cfg.layers), max_length=4, draft_len=2, constraint=_choices())
    with pytest.raises(ValueError):
        _session(model, 4, use_graph=False, constraint=_choices(), constraint_states=[0, 0])             # one start state per sample
    with pytest.raises(ValueError):
        _session(model, 4, use_graph=False, constraint=_choices(), constraint_states=[0, 0, 99])
    with pytest.raises(ValueError):
        _session(model, 4, use_graph=False, constraint="yes no")


# ----------------------------------------------------------------------------- the batcher
LONG = [[30, 31, 32, 33, 34, 35], [30, 31, 32, 40, 41, 42], [30, 36, 37, 38, 39, 43], [44, 45, 46, 47, 48, 49]]


@pytest.mark.parametrize("grow", [False, True])
def test_batcher_serves_constrained_and_free_requests(model, grow):
    """7 requests on 3 slots: 4 decode under two named automata, 3 are free.  check_every = 2 and six-token choices keep a constrained
    request in flight over several rounds; with grow, the fourth request's prompt is longer than the slots' reserve, so the cache
    grows and the step is re-captured while request 0 is in the middle of its choice - it must go on from its state, not from the root."""
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.constraints import TokenAutomaton
    from unimedvl_amd.serving import ContinuousBatcher
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    ident = lambda x: x   # noqa: E731
    named = {"long": TokenAutomaton.from_choices(LONG, EOS), "short": TokenAutomaton.from_choices(CHOICES, EOS)}
    texts = {"long": [" ".join(map(str, c)) for c in LONG], "short": [" ".join(map(str, c)) for c in CHOICES]}
    big = " ".join(str(5 + i % 250) for i in range(300 if grow else 12))
    reqs = [("5 17 40 23", "long", 10), ("200 31 7", None, 2), ("9 8 7 6", "short", 10), (big, None, 6), ("61 62", "long", 10),
            ("70 71 72", None, 5), ("15 16", "short", 10)]
    kw = dict(slots=3, max_context=64, max_new_tokens=10, check_every=2)
    srv = ContinuousBatcher(model, tok, NEW_TOKEN_IDS, ident, constraints=named, **kw)
    rids = [srv.submit([], prompt, max_new_tokens=n, constraint=name) for prompt, name, n in reqs]
    got = srv.run()
    assert (srv.stats["cache_grows"] > 0) == grow, srv.stats
    for rid, (prompt, name, n) in zip(rids, reqs):
        if name is not None:
            assert got[rid].strip() in texts[name], f"request {rid} under {name!r}: {got[rid]!r}"
    # the same seven requests, all free, through a batcher built without constraints (the same admission order, so the big prompt
    # arrives after the first round there too)
    plain = ContinuousBatcher(model, tok, NEW_TOKEN_IDS, ident, **kw)
    pids = [plain.submit([], prompt, max_new_tokens=n) for prompt, name, n in reqs]
    want = plain.run()
    for rid, pid, (prompt, name, n) in zip(rids, pids, reqs):
        if name is None:
            assert got[rid] == want[pid], f"free request {rid}: {got[rid]!r} in the batcher with constraints, {want[pid]!r} without"
        else:
            assert want[pid].strip() not in texts[name], "an unconstrained answer is already a choice: the test shows nothing"
    with pytest.raises(ValueError, match="constraint"):
        srv.submit([], "5", constraint="nope")
    with pytest.raises(ValueError, match="constraint"):
        plain.submit([], "5", constraint="long")
