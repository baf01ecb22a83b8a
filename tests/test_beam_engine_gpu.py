"""Beam search decode through the engine (unimedvl_amd/beam.py, Bagel.generate_text / chat, VQAInferencer), at the tiny configuration:
every returned hypothesis replayed through a plain forced session, the whole search against tests/beam_ref.py driven by the plain
engine, one beam against greedy decode, graph replay against eager steps, finished hypotheses, the public interface."""
import functools

import numpy as np
import pytest
import torch

import beam_ref as R
from conftest import NEW_TOKEN_IDS
from test_logprob_gpu import model  # noqa: F401  (the tiny engine fixture)

pytestmark = pytest.mark.gpu
BOUND = 1e-4          # of a log-probability (include/unimedvl_hip.h, token log-probabilities)
PROMPTS = [[11, 22, 33, 44, 55], [66, 77, 88]]
B, K, STEPS = 2, 3, 12


def _ctx(model, prompts=PROMPTS, paged=True):
    """a freshly prefilled cache of the prompts' text contexts and the start tokens"""
    from unimedvl_amd.kvcache import NaiveCache, PagedCache

    class Tok:
        def encode(self, s):
            return prompts[int(s)]
    n = len(prompts)
    cache = PagedCache(model.cfg.layers, pool_pages=96, max_context=2048) if paged else NaiveCache(model.cfg.layers)
    gi, kvl, rope = model.prepare_prompts([0] * n, [0] * n, [str(i) for i in range(n)], Tok(), NEW_TOKEN_IDS)
    with torch.no_grad():
        cache = model.forward_cache_update_text(cache, **gi)
    return cache, model.prepare_start_tokens(kvl, rope, NEW_TOKEN_IDS)


def _beam(model, steps=STEPS, k=K, **kw):
    from unimedvl_amd.beam import BeamDecodeSession
    cache, gi = _ctx(model)
    with torch.no_grad():
        return cache, gi, BeamDecodeSession(model.language_model, cache, gi["packed_start_tokens"], gi["packed_query_position_ids"], steps, k, **kw)


@functools.lru_cache(maxsize=None)
def _end_token(model):
    """an end token from the model's own step-2 candidates, so that hypotheses finish before max_length"""
    _, _, sess = _beam(model, use_graph=False)
    with torch.no_grad():
        sess.step(3)
    tok = int(sess.beam.cand_ids[0, 0])                   # request 0's best beam's best candidate: first in its order
    sess.release()
    return tok


@functools.lru_cache(maxsize=None)
def _searched(model, use_graph=True, early=False, lp=1.0):
    """one whole search with every hypothesis returned: (result, nsplit, pages in use before / during / after)"""
    cache, gi, sess = _beam(model, end_token_id=_end_token(model), num_return_sequences=K, use_graph=use_graph, early_stopping=early,
                            length_penalty=lp, eos_check_every=4)
    during = cache.pages_in_use()
    with torch.no_grad():
        res = sess.run().result()
    nsplit, steps = sess.nsplit, sess.steps_done
    sess.release()
    return res, nsplit, steps, (during, cache.pages_in_use())


def test_finished_hypotheses_occur_and_pages_come_back(model):
    res, _, steps, (during, after) = _searched(model)
    eos = _end_token(model)
    ended = [h for hyps in res for h in hyps if h["tokens"][-1] == eos and len(h["tokens"]) < STEPS]
    assert ended, "no hypothesis finished before max_length"
    assert all(h["tokens_no_end"] == h["tokens"][:-1] and eos not in h["tokens"][:-1] for h in ended)
    assert after == B and during > after                  # one prompt page per request; the fork's pages came back
    for hyps in res:
        assert len(hyps) == K and [h["score"] for h in hyps] == sorted((h["score"] for h in hyps), reverse=True)
        for h in hyps:
            assert len(h["logprobs"]) == len(h["tokens"]) <= STEPS
            assert abs(sum(np.float32(v) for v in h["logprobs"]) - h["total"]) <= 1e-4 * len(h["tokens"])
            assert h["score"] == pytest.approx(h["total"] / len(h["tokens"]), rel=1e-6)


def test_hypotheses_replay_through_a_forced_session(model):
    """each hypothesis as one row of a plain forced session with the same row count and nsplit on a fresh fork of the prompt:
    the same kernels over the same rows, so the per-token log-probabilities are expected bit-equal"""
    from unimedvl_amd.decode import DecodeSession
    res, nsplit, _, _ = _searched(model)
    cache, gi = _ctx(model)
    fork = cache.fork_beams(K, STEPS + 1)
    forced = torch.full((STEPS, B * K), -1, dtype=torch.int64)
    for b, hyps in enumerate(res):
        for i, h in enumerate(hyps):
            forced[:len(h["tokens"]), b * K + i] = torch.tensor(h["tokens"])
    with torch.no_grad():
        sess = DecodeSession(model.language_model, fork, gi["packed_start_tokens"].repeat_interleave(K),
                             gi["packed_query_position_ids"].repeat_interleave(K), STEPS, forced_ids=forced, logprobs=True, nsplit=nsplit)
        sess.step(STEPS)
    got = sess.pred_logprobs.cpu()
    worst, differ = 0.0, 0
    for b, hyps in enumerate(res):
        for i, h in enumerate(hyps):
            want = torch.tensor(h["logprobs"], dtype=torch.float32)
            mine = got[:len(want), b * K + i]
            worst = max(worst, float((mine.double() - want.double()).abs().max()))
            differ += int((mine.view(torch.int32) != want.view(torch.int32)).sum())
    print(f"forced replay: {differ} log-probabilities differ in bits, max |difference| {worst:.3g}")
    fork.release_all()
    assert differ == 0, (differ, worst)


def test_the_search_is_beam_ref_over_the_plain_engine(model):
    """beam_ref driven by the plain engine (eager forced sessions over K copies of a request's prompt) as its model function"""
    from unimedvl_amd.decode import DecodeSession
    eos = _end_token(model)
    res, nsplit, _, _ = _searched(model, use_graph=False)

    def engine(b):
        def fn(prefixes):
            cache, gi = _ctx(model, [PROMPTS[b]] * K, paged=False)
            n = len(prefixes[0])
            forced = torch.full((n + 1, K), -1, dtype=torch.int64)
            if n:
                forced[:n] = torch.tensor(prefixes).t()
            with torch.no_grad():
                sess = DecodeSession(model.language_model, cache, gi["packed_start_tokens"], gi["packed_query_position_ids"], n + 1,
                                     forced_ids=forced, use_graph=False, nsplit=nsplit)
                sess.step(n + 1)
            return torch.log_softmax(sess.logits.float(), -1).cpu().numpy()
        return fn
    for b in range(B):
        want = R.search(engine(b), K, STEPS, eos, length_penalty=1.0, early_stopping=False).hypotheses()
        assert [h["tokens"] for h in res[b]] == [h["tokens"] for h in want]
        for g, w in zip(res[b], want):
            assert abs(g["total"] - w["total"]) <= BOUND * len(g["tokens"]) and abs(g["score"] - w["score"]) <= BOUND


def test_graph_replay_is_the_eager_search(model):
    for early, lp in ((False, 1.0), (True, 0.0), (False, 2.0)):
        a, b = _searched(model, True, early, lp), _searched(model, False, early, lp)
        assert a[0] == b[0] and a[2] == b[2], (early, lp)


def test_one_beam_is_greedy(model):
    from unimedvl_amd.beam import BeamDecodeSession
    from unimedvl_amd.decode import DecodeSession
    cache, gi = _ctx(model)
    with torch.no_grad():
        one = BeamDecodeSession(model.language_model, cache, gi["packed_start_tokens"], gi["packed_query_position_ids"], 8, 1, end_token_id=301)
    assert type(one) is DecodeSession
    with torch.no_grad():
        one.step(8)
        want = model.generate_text(past_key_values=_ctx(model)[0], max_length=8, **gi)
        got = model.generate_text(past_key_values=_ctx(model)[0], max_length=8, num_beams=1, length_penalty=2.0, **gi)
    assert torch.equal(got, want) and torch.equal(one.in_ids, want)


def test_generate_text_returns_the_best_hypotheses(model):
    eos = _end_token(model)
    res, _, _, _ = _searched(model)
    cache, gi = _ctx(model)
    lens = list(cache.lens)
    with torch.no_grad():
        ids, lps = model.generate_text(past_key_values=cache, max_length=STEPS, end_token_id=eos, num_beams=K, return_logprobs=True,
                                       num_return_sequences=2, **gi)
    assert cache.lens == lens and cache.pages_in_use() == B, "the prompt's cache is left as it was"
    assert ids.shape[1] == B and ids.shape[0] == 1 + max(len(h[0]["tokens"]) for h in res) and lps.shape == (ids.shape[0] - 1, B)
    assert torch.equal(ids[0].cpu(), gi["packed_start_tokens"].cpu())
    for b in range(B):
        best = res[b][0]
        n = len(best["tokens"])
        assert ids[1:n + 1, b].tolist() == best["tokens"] and (ids[n + 1:, b] == eos).all()
        assert lps[:n, b].tolist() == [float(np.float32(v)) for v in best["logprobs"]] and (lps[n:, b] == 0).all()
        assert [h["tokens"] for h in model.last_beam_hypotheses[b]] == [h["tokens"] for h in res[b][:2]]


def test_chat_and_the_inferencer_key(model):
    from PIL import Image
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.interactive_vqa_inferencer import VQAInferencer
    from unimedvl_amd.transforms import ImageTransform
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    ident = lambda x: x  # noqa: E731
    answer = model.chat(tok, NEW_TOKEN_IDS, ident, [], "5 17 40 23", max_length=10, num_beams=3)
    best = model.last_beam_hypotheses[0][0]
    assert answer == "".join(f" {t}" for t in best["tokens_no_end"]) and all(t != 301 for t in best["tokens_no_end"])
    a2, ids, lps = model.chat(tok, NEW_TOKEN_IDS, ident, [], "5 17 40 23", max_length=10, num_beams=3, return_logprobs=True)
    assert a2 == answer and ids == best["tokens_no_end"] and len(lps) == len(ids)
    pairs = model.chat(tok, NEW_TOKEN_IDS, ident, [], "5 17 40 23", max_length=10, num_beams=3, num_return_sequences=3)
    assert len(pairs) == 3 and pairs[0][0] == answer and [s for _, s in pairs] == sorted((s for _, s in pairs), reverse=True)
    pil = Image.fromarray(np.random.default_rng(3).integers(0, 255, (60, 84, 3), dtype=np.uint8))

    def make(**cfg):
        v = VQAInferencer(dict({"max_new_tokens": 10, "do_sample": False}, **cfg))
        v.load_model(model=model, tokenizer=tok, new_token_ids=NEW_TOKEN_IDS)
        v.image_transform = ImageTransform(56, 28, 14)
        return v
    res = make(num_beams=3, num_return_sequences=2).infer_single(pil, "5 6 7 8")
    want = model.chat(tok, NEW_TOKEN_IDS, ImageTransform(56, 28, 14), [pil], "5 6 7 8", max_length=10, num_beams=3)
    assert res["answer"] == want and len(res["answers"]) == 2 and res["answers"][0][0] == want
    assert make(num_beams=3).infer_single(pil, "5 6 7 8")["answer"] == want


def test_refusals(model):
    cache, gi = _ctx(model, paged=False)
    with pytest.raises(ValueError, match="PagedCache"):
        model.generate_text(past_key_values=cache, max_length=4, num_beams=3, **gi)
    cache, gi = _ctx(model)
    for bad in (dict(do_sample=True), dict(top_logprobs=2), dict(return_logits=True), dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2),
                dict(draft_len=2), dict(logit_bias={5: -1.0}), dict(top_k=4, do_sample=True), dict(num_beams=11), dict(num_return_sequences=4),
                dict(early_stopping="never")):
        with pytest.raises(ValueError):
            model.generate_text(past_key_values=cache, max_length=4, **{**dict(num_beams=3), **bad}, **gi)
    assert cache.pages_in_use() == B
    with pytest.raises(ValueError, match="choices"):
        from oracle.toy_tokenizer import ToyTokenizer
        model.chat(ToyTokenizer(NEW_TOKEN_IDS), NEW_TOKEN_IDS, lambda x: x, [], "5 17", max_length=4, num_beams=2, choices=["1", "2"])
