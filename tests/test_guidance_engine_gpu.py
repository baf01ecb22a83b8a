"""Classifier-free guidance for text through the engine at the tiny configuration (B = 3 requests, 6 rows, 16 steps, eager and graph).

The replay check: the guided session's tokens are fed, through forced_ids, to a PLAIN six-row session over the same contexts - both
rows of a pair the pair's token.  A row's logits do not depend on what the other rows hold, so the plain session's stored logits are
the guided session's logits before the stage; the numpy model of the definition (tests/guidance_ref.py), given the lse[] words the
guided session's stage wrote at that step, must then give the guided session's logits bit for bit, and the guided token is their
lowest-column argmax - at every step, no margin.  The only tolerance is the header's 1e-4 on a log-probability."""
import numpy as np
import pytest
import torch

import guidance_ref as G
import penalty_ref as P
from conftest import NEW_TOKEN_IDS

pytestmark = pytest.mark.gpu
T = 0.7
STEPS = 16
B = 3
COND = [[11, 22, 33, 44, 55], [66, 77, 88], [99, 111, 122, 133]]
UNCOND = [[11, 22], [201, 77, 88, 14, 15], [133, 122, 111]]          # other tokens, other lengths
SCALES = [3.0, 1.5, 0.5]
BETAS = [0.0, 0.1, 0.0]
BOUND = 1e-4          # of a log-probability (include/unimedvl_hip.h, token log-probabilities)


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
    monkeypatch.setenv("UMV_DECODE_NSPLIT", "2")      # a row's logits do not depend on the session it is served in


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _context(model, prompts):
    """(prefilled cache, start-token inputs) of one text context per request"""
    from unimedvl_amd.kvcache import NaiveCache

    class Tok:
        def encode(self, s):
            return prompts[int(s)]
    n = len(prompts)
    gi, kvl, rope = model.prepare_prompts([0] * n, [0] * n, [str(i) for i in range(n)], Tok(), NEW_TOKEN_IDS)
    cache = model.forward_cache_update_text(NaiveCache(model.cfg.layers), **gi)
    return cache, model.prepare_start_tokens(kvl, rope, NEW_TOKEN_IDS)


def _merged(model, steps):
    from unimedvl_amd.kvcache import NaiveCache
    (cc, gc), (cu, gu) = _context(model, COND), _context(model, UNCOND)
    both = NaiveCache.merged([cc, cu], [B, B], steps + 1, model.cfg.kv_heads, model.cfg.head_dim, model.device)
    return both, gc, gu


def _guided(model, steps=STEPS, scales=SCALES, betas=BETAS, **kw):
    from unimedvl_amd.guidance import GuidedDecodeSession
    both, gc, gu = _merged(model, steps)
    with torch.no_grad():
        return GuidedDecodeSession(model.language_model, both, gc["packed_start_tokens"], gc["packed_query_position_ids"], steps, scales,
                                   guidance_positions=gu["packed_query_position_ids"], guidance_plausibility=betas, **kw)


def _plain(model, steps, forced, **kw):
    from unimedvl_amd.decode import DecodeSession
    both, gc, gu = _merged(model, steps)
    with torch.no_grad():
        return DecodeSession(model.language_model, both, gc["packed_start_tokens"].repeat(2),
                             torch.cat([gc["packed_query_position_ids"], gu["packed_query_position_ids"]]), steps, use_graph=False,
                             forced_ids=forced, **kw)


def _run(sess, steps):
    """step by step: the logits and the lse words every step left"""
    logits, lse = [], []
    with torch.no_grad():
        for _ in range(steps):
            sess.step(1)
            logits.append(_bits(sess.logits))
            if getattr(sess, "guid", None) is not None:
                lse.append(sess.lse.cpu().numpy().copy())
    torch.cuda.synchronize()
    return logits, lse


def _replay(model, use_graph, **sampler):
    a = _guided(model, use_graph=use_graph, logprobs=True, **sampler)
    assert (a.graph is not None) == use_graph and a.guid is not None and a.rows == 2 * B
    a_logits, a_lse = _run(a, STEPS)
    assert torch.equal(a.pred_ids[:, B:], a.pred_ids[:, :B]) and torch.equal(a.in_ids[:, B:], a.in_ids[:, :B]), \
        "the unconditional rows were not fed their partners' tokens"
    b = _plain(model, STEPS, a.pred_ids.clone(), **sampler)
    b_logits, _ = _run(b, STEPS)
    assert torch.equal(a.in_ids, b.in_ids), "the plain session was fed other tokens"
    lb = [G.log_beta(v) for v in BETAS]
    temp = sampler.get("temperature", 0.0) if sampler.get("do_sample") else 0.0
    lp = a.token_logprobs().cpu().numpy()
    worst = 0.0
    for s in range(STEPS):
        for r in range(B):
            want = G.combine_row(b_logits[s][r], b_logits[s][B + r], a_lse[s][r], a_lse[s][B + r], SCALES[r], lb[r])
            assert P.same_bits(a_logits[s][r], want).all(), f"step {s} request {r}: the guided logits are not the model's"
            assert np.array_equal(a_logits[s][B + r], b_logits[s][B + r]), f"step {s} request {r}: the unconditional row moved"
            assert abs(float(a_lse[s][r]) - G.lse64(b_logits[s][r])) <= BOUND and abs(float(a_lse[s][B + r]) - G.lse64(b_logits[s][B + r])) <= BOUND
            tok = int(a.tokens()[s, r])
            if temp == 0:
                v = P.bf16_float(want).astype(np.float64)
                assert tok == int(np.flatnonzero(v == v.max())[0]), f"step {s} request {r}: token {tok} is not the argmax of the guided row"
            else:
                assert want[tok] != G.NINF, f"step {s} request {r}: a dropped column was drawn"
            worst = max(worst, abs(float(lp[s, r]) - P.logprob(want, tok, temp)))
    print(f"log-probabilities off the fp64 log-softmax of the combined row by at most {worst:.3g}")
    assert worst <= BOUND
    return a


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_replay_step_by_step(model, use_graph):
    a = _replay(model, use_graph)
    assert a.step_end == "logprob" and a.guid["stats"] is None, "a greedy session reads the epilogue's own statistics"


def test_replay_sampled_with_truncation(model):
    a = _replay(model, True, do_sample=True, temperature=T, seed=77, top_p=0.9)
    assert a.step_end == "truncated" and a.guid["stats"] is not None


def test_graph_and_eager_are_bit_identical(model):
    for kw in ({}, dict(do_sample=True, temperature=T, seed=5, top_k=20)):
        runs = []
        for use_graph in (False, True):
            s = _guided(model, use_graph=use_graph, logprobs=True, top_logprobs=3, **kw)
            with torch.no_grad():
                s.step(STEPS)
            runs.append((s.tokens().clone(), s.token_logprobs().clone(), s.lse.clone(), s.top()[0].clone(), s.top()[1].clone()))
        for e, g in zip(*runs):
            assert torch.equal(e.view(torch.int32) if e.dtype == torch.float32 else e, g.view(torch.int32) if g.dtype == torch.float32 else g)


def _generate(model, cc, gc, cu=None, gu=None, **kw):
    extra = {}
    if cu is not None:
        extra = dict(guidance_past_key_values=cu, guidance_query_position_ids=gu["packed_query_position_ids"])
    return model.generate_text(past_key_values=cc, max_length=STEPS, **gc, **extra, **kw)


def test_generate_text(model):
    (cc, gc), (cu, gu) = _context(model, COND), _context(model, UNCOND)
    lens = (list(cc.lens), list(cu.lens))
    plain = _generate(model, cc.snapshot(), gc)
    same = _generate(model, cc.snapshot(), gc, guidance_scale=1.0)
    assert torch.equal(plain, same), "guidance_scale = 1.0 is the plain call"
    out = _generate(model, cc, gc, cu, gu, guidance_scale=3.0)
    assert (list(cc.lens), list(cu.lens)) == lens, "both caches keep their lengths"
    assert tuple(out.shape) == (STEPS, B) and torch.equal(out[0], plain[0])
    assert not torch.equal(out, plain), "guidance_scale = 3 against another context changed no token: the test shows nothing"
    # the session behind it, token for token
    s = _guided(model, scales=3.0, betas=0.0, use_graph=True)
    with torch.no_grad():
        s.step(STEPS)
    assert torch.equal(out, s.fed(STEPS))
    # sampled, truncated, with log-probabilities and alternatives: shapes, reproducible, the fed token's entry is its log-probability
    kw = dict(guidance_scale=1.5, guidance_plausibility=0.1, do_sample=True, temperature=T, top_p=0.9, return_logprobs=True, top_logprobs=3)
    torch.manual_seed(3)
    ids, lp, top = _generate(model, cc, gc, cu, gu, **kw)
    torch.manual_seed(3)
    ids2, lp2, top2 = _generate(model, cc, gc, cu, gu, **kw)
    assert torch.equal(ids, ids2) and torch.equal(lp, lp2) and torch.equal(top.ids, top2.ids)
    assert tuple(ids.shape) == (STEPS, B) and tuple(lp.shape) == (STEPS, B) and tuple(top.ids.shape) == (STEPS, B, 3)
    hit = top.ids[:-1] == ids[1:].unsqueeze(-1).to(torch.int32)
    assert bool(hit.any()) and torch.equal(top.logprobs[:-1][hit], lp[:-1].unsqueeze(-1).expand(-1, -1, 3)[hit])
    # per_sample_eos: the batch stops when every request has emitted the end token - here a token request 0 emits at its first step
    first = int(out[1, 0])
    short = _generate(model, cc, gc, cu, gu, guidance_scale=3.0, end_token_id=first)
    assert short.shape[0] == 1 and (list(cc.lens), list(cu.lens)) == lens
    each = _generate(model, cc, gc, cu, gu, guidance_scale=3.0, end_token_id=first, per_sample_eos=True)
    assert each.shape[0] >= 1 and torch.equal(each, out[:each.shape[0]])


def test_chat_and_the_inferencers_keys(model):
    from PIL import Image
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.interactive_vqa_inferencer import VQAInferencer
    from unimedvl_amd.kvcache import NaiveCache
    from unimedvl_amd.transforms import ImageTransform
    tok = ToyTokenizer(NEW_TOKEN_IDS)
    ident = lambda x: x   # noqa: E731
    image = torch.randn(3, 42, 56, generator=torch.Generator().manual_seed(21)).clamp(-1, 1)
    prompt, negative, n = "5 17 40 17", "9 8 7", 12

    def by_hand(images, text, unconditional, **kw):
        """chat's own prefill, then generate_text on the two contexts"""
        cache, lens, rope = NaiveCache(model.cfg.layers), [0], [0]
        for im in images:
            gi, lens, rope = model.prepare_vit_images(lens, rope, [im], ident, NEW_TOKEN_IDS)
            cache = model.forward_cache_update_vit(cache, **gi)
        gi, lens, rope = model.prepare_prompts(lens, rope, [text], tok, NEW_TOKEN_IDS)
        cache = model.forward_cache_update_text(cache, **gi)
        start = model.prepare_start_tokens(lens, rope, NEW_TOKEN_IDS)
        ugi, ulens, urope = model.prepare_prompts([0], [0], [unconditional], tok, NEW_TOKEN_IDS)
        ucache = model.forward_cache_update_text(NaiveCache(model.cfg.layers), **ugi)
        ustart = model.prepare_start_tokens(ulens, urope, NEW_TOKEN_IDS)
        ids = model.generate_text(past_key_values=cache, max_length=n, end_token_id=NEW_TOKEN_IDS["eos_token_id"],
                                  guidance_past_key_values=ucache, guidance_query_position_ids=ustart["packed_query_position_ids"],
                                  **start, **kw)
        return tok.decode(ids[:, 0].cpu()).split("<|im_end|>")[0].split("<|im_start|>")[1]
    with torch.no_grad():
        plain = model.chat(tok, NEW_TOKEN_IDS, ident, [image], prompt, max_length=n)
        dropped = model.chat(tok, NEW_TOKEN_IDS, ident, [image], prompt, max_length=n, guidance_scale=3.0)
        assert dropped == by_hand([image], prompt, prompt, guidance_scale=3.0), "negative_prompt=None: the same prompt without its images"
        neg = model.chat(tok, NEW_TOKEN_IDS, ident, [image], prompt, max_length=n, guidance_scale=3.0, negative_prompt=negative,
                         guidance_plausibility=0.1)
        assert neg == by_hand([image], prompt, negative, guidance_scale=3.0, guidance_plausibility=0.1)
        text_only = model.chat(tok, NEW_TOKEN_IDS, ident, [], prompt, max_length=n, guidance_scale=3.0, negative_prompt=negative)
        assert text_only == by_hand([], prompt, negative, guidance_scale=3.0)
        assert len({plain, dropped, neg}) > 1, "guidance changed no answer: the test shows nothing"
        answer, ids, lps = model.chat(tok, NEW_TOKEN_IDS, ident, [image], prompt, max_length=n, guidance_scale=3.0, return_logprobs=True)
        assert answer == dropped and len(ids) == len(lps) and all(v <= 0 for v in lps)
        with pytest.raises(ValueError, match="nothing to contrast"):
            model.chat(tok, NEW_TOKEN_IDS, ident, [], prompt, max_length=n, guidance_scale=3.0)
        with pytest.raises(ValueError, match="negative_prompt"):
            model.chat(tok, NEW_TOKEN_IDS, ident, [image], prompt, max_length=n, negative_prompt=negative)
        with pytest.raises(ValueError, match="choices"):
            model.chat(tok, NEW_TOKEN_IDS, ident, [image], prompt, max_length=n, guidance_scale=3.0, choices=["10 11", "20"])
        pil = Image.fromarray(np.random.default_rng(3).integers(0, 255, (60, 84, 3), dtype=np.uint8))

        def make(**cfg):
            v = VQAInferencer(dict({"max_new_tokens": 8, "do_sample": False}, **cfg))
            v.load_model(model=model, tokenizer=tok, new_token_ids=NEW_TOKEN_IDS)
            v.image_transform = ImageTransform(56, 28, 14)
            return v
        tr = ImageTransform(56, 28, 14)
        for cfg in (dict(guidance_scale=3.0), dict(guidance_scale=3.0, negative_prompt=negative, guidance_plausibility=0.1)):
            got = make(**cfg).infer_single(pil, "5 6 7 8")["answer"]
            want = model.chat(tok, NEW_TOKEN_IDS, tr, [pil.convert("RGB")], "5 6 7 8", max_length=8, **cfg)
            assert got == want, cfg
        with pytest.raises(ValueError, match="num_beams"):
            make(guidance_scale=3.0, num_beams=2).infer_single(pil, "5 6 7 8")


def test_refusals(model, monkeypatch):
    from unimedvl_amd.constraints import TokenAutomaton
    from unimedvl_amd.kvcache import PagedCache
    from unimedvl_amd.sampling import SamplingParams
    (cc, gc), (cu, gu) = _context(model, COND), _context(model, UNCOND)
    lens = (list(cc.lens), list(cu.lens))
    on = dict(guidance_scale=3.0)
    refused = [dict(num_beams=2), dict(draft_len=2), dict(sampling=SamplingParams()), dict(repetition_penalty=1.2), dict(presence_penalty=0.5),
               dict(frequency_penalty=0.5), dict(logit_bias={3: 1.0}), dict(no_repeat_ngram_size=2),
               dict(constraint=TokenAutomaton.from_allowed_tokens([5, 7])), dict(bad_words_ids=[[1, 2]]), dict(suppress_tokens=[4]),
               dict(begin_suppress_tokens=[4]), dict(min_new_tokens=3, end_token_id=2), dict(return_logits=True)]
    for kw in refused:
        with pytest.raises(ValueError, match=next(iter(kw))):
            _generate(model, cc, gc, cu, gu, **on, **kw)
    for kw in (dict(row_sampling=[SamplingParams()] * B), dict(forced_ids=torch.zeros((4, 2 * B), dtype=torch.int64)), dict(constraint=object())):
        with pytest.raises(ValueError, match=next(iter(kw))):
            _guided(model, 4, **kw)
    with pytest.raises(TypeError):
        _guided(model, 4, no_such_keyword=1)
    for bad in (dict(guidance_scale=-1.0), dict(guidance_scale=float("nan")), dict(guidance_scale=3.0, guidance_plausibility=1.0),
                dict(guidance_scale=1.0, guidance_plausibility=0.5)):
        with pytest.raises(ValueError):
            _generate(model, cc, gc, cu, gu, **bad)
    with pytest.raises(ValueError, match="guidance_past_key_values"):
        _generate(model, cc, gc, **on)                                              # no unconditional contexts
    with pytest.raises(ValueError, match="guidance_scale"):
        _generate(model, cc, gc, cu, gu)                                            # ... and contexts without a scale
    two = _context(model, UNCOND[:2])
    with pytest.raises(ValueError, match="same number"):
        _generate(model, cc, gc, *two, **on)
    with pytest.raises(ValueError, match="PagedCache"):
        _generate(model, cc, gc, PagedCache(model.cfg.layers, pool_pages=8, max_context=64), gu, **on)
    with pytest.raises(ValueError, match="PagedCache"):
        _generate(model, PagedCache(model.cfg.layers, pool_pages=8, max_context=64), gc, cu, gu, **on)
    monkeypatch.setenv("UMV_DECODE_FUSED_ARGMAX", "0")
    with pytest.raises(ValueError, match="UMV_DECODE_FUSED_ARGMAX"):
        _generate(model, cc, gc, cu, gu, **on)
    with pytest.raises(ValueError, match="UMV_DECODE_FUSED_ARGMAX"):
        _guided(model, 4)
    monkeypatch.undo()
    assert (list(cc.lens), list(cu.lens)) == lens, "a refused call touched a cache"
    s = _guided(model, 4, use_graph=False)
    with pytest.raises(RuntimeError):
        s.set_slot(0, 1, 1, 1)
