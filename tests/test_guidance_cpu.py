"""Classifier-free guidance for text (include/unimedvl_hip.h) without a GPU: the numpy model of the definition (tests/guidance_ref.py)
against torch's log_softmax and against HF's own UnbatchedClassifierFreeGuidanceLogitsProcessor, the fp32 chain against the fp64 form,
the plausibility floor, and the keyword surface with the refusals that need no launch."""
import inspect
import math
import os

import numpy as np
import pytest
import torch

import guidance_ref as G
import penalty_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = [0.0, 0.5, 1.0, 1.5, 3.0]


def _rows(V, seed, ties=False, ninf=False):
    rng = np.random.default_rng(seed)
    c = P.bf16_bits((rng.standard_normal(V) * 3).astype(np.float32))
    u = P.bf16_bits((rng.standard_normal(V) * 3).astype(np.float32))
    if ties:
        c[rng.choice(V, V // 4, replace=False)] = P.bf16_bits(np.array([1.5], dtype=np.float32))[0]
        u[rng.choice(V, V // 4, replace=False)] = c[3]
    if ninf:
        c[rng.choice(V, V // 5, replace=False)] = G.NINF
    return c, u


def _f32(x):
    return np.float32(x)


def test_fp64_form_is_the_formula_on_log_softmaxes():
    for seed, V in ((1, 330), (2, 4152)):
        c, u = _rows(V, seed)
        tc = torch.from_numpy(P.bf16_float(c).astype(np.float64))
        tu = torch.from_numpy(P.bf16_float(u).astype(np.float64))
        for g in SCALES:
            want = g * (torch.log_softmax(tc, -1) - torch.log_softmax(tu, -1)) + torch.log_softmax(tu, -1)
            got = G.combine64(c, u, g)
            assert np.allclose(got, want.numpy(), rtol=0, atol=1e-12), f"V={V} g={g}"


@pytest.mark.parametrize("case", ["random", "ties", "-inf in the conditional row"])
def test_model_equals_hf_processor(case):
    transformers = pytest.importorskip("transformers")
    from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor as Proc
    V = 330
    c, u = _rows(V, 7, ties=case == "ties", ninf=case.startswith("-inf"))
    fc, fu = torch.from_numpy(P.bf16_float(c)).reshape(1, V), torch.from_numpy(P.bf16_float(u)).reshape(1, V)

    class Out(dict):
        logits = None

    class Stub:                       # a model that returns fixed unconditional logits for the last position
        def __call__(self, input_ids, **kw):
            out = Out()
            out.logits = fu.reshape(1, 1, V).expand(1, input_ids.shape[1], V)
            return out
    ids = torch.tensor([[5, 6, 7]])
    lse_c, lse_u = _f32(G.lse64(c)), _f32(G.lse64(u))
    for g in SCALES:
        proc = Proc(g, Stub(), unconditional_ids=ids, use_cache=False)
        hf = proc(ids, fc.clone())[0].numpy()                                         # fp32
        if g == 1.0:                                                                  # HF returns log_softmax: the same distribution,
            assert np.allclose(hf, (P.bf16_float(c) - lse_c), rtol=0, atol=2e-6, equal_nan=True)      # and the stage leaves the row alone
            continue
        ref64 = G.combine64(c, u, g)
        fin = np.isfinite(ref64)
        if g == 0.0:                  # HF's arithmetic gives 0 * -inf = NaN on a banned column; the definition keeps it banned
            assert np.isnan(hf[np.isneginf(ref64)]).all() and not np.isnan(hf[fin]).any()
            hf = np.where(np.isneginf(ref64), -np.inf, hf)
        assert np.array_equal(np.isneginf(ref64), np.isneginf(hf)), f"{case} g={g}: -inf columns"
        # within fp32 rounding of values of magnitude <= ~64: a few ulps of 2^-18
        assert np.abs(hf[fin] - ref64[fin]).max() <= 1e-4, f"{case} g={g}"
        # ... and the bf16 result of the fp32 chain is the bf16 neighbourhood of HF's fp32 value
        got = P.bf16_float(G.combine_row(c, u, lse_c, lse_u, g)).astype(np.float64)
        assert np.array_equal(np.isneginf(got), np.isneginf(hf))
        assert (np.abs(got[fin] - hf[fin]) <= np.abs(hf[fin]) * 2.0 ** -8 + 1e-4).all(), f"{case} g={g}: bf16 of the chain"


def test_fp32_chain_is_within_one_bf16_value_of_the_fp64_form():
    total = equal = 0
    for seed, V in ((11, 330), (12, 4152), (13, 40)):
        c, u = _rows(V, seed, ninf=seed == 12)
        lse_c, lse_u = _f32(G.lse64(c)), _f32(G.lse64(u))
        for g in SCALES:
            got = G.combine_row(c, u, lse_c, lse_u, g)
            want = P.bf16_bits(G.combine64(c, u, g).astype(np.float32))
            # neighbours in bf16: the order-preserving integer images differ by at most 1
            gi, wi = got.astype(np.int32), want.astype(np.int32)
            key = lambda b: np.where(b & 0x8000, 0x8000 - (b & 0x7FFF), 0x8000 + b)      # noqa: E731
            assert (np.abs(key(gi) - key(wi)) <= 1).all(), f"V={V} g={g}"
            total += V
            equal += int((got == want).sum())
    print(f"fp32 chain bit-equal to bf16(fp64 form) on {equal / total:.4%} of {total} columns")
    assert equal / total > 0.9


def test_edge_cases_of_the_definition():
    V = 40
    c, u = _rows(V, 21)
    c[3], u[4], c[5], u[6] = G.NINF, G.NINF, 0x7FC0, 0x7FC0
    c[7], u[7] = G.NINF, 0x7FC0
    lse_c, lse_u = _f32(2.5), _f32(3.25)                     # (any words: the chain takes them as given)
    out = G.combine_row(c, u, lse_c, lse_u, 3.0)
    assert out[3] == G.NINF and out[7] == G.NINF, "a banned column stays banned"
    assert out[4] == P.bf16_bits(np.array([P.bf16_float(c[4:5])[0] - lse_c], dtype=np.float32))[0], "no opinion: bf16(c)"
    f = P.bf16_float(out)
    assert np.isnan(f[5]) and np.isnan(f[6]), "a NaN in either row gives NaN"
    dead = np.full(V, G.NINF, dtype=np.uint16)
    assert np.array_equal(G.combine_row(dead, u, lse_c, lse_u, 3.0), dead), "a conditional row of -inf only is left as it is"
    assert np.isnan(G.lse64(c)) and G.lse64(dead) == -np.inf


@pytest.mark.parametrize("beta", [0.0, 0.1, 0.9])
def test_plausibility_floor(beta):
    V = 330
    c, u = _rows(V, 31, ties=True)
    lse_c, lse_u = _f32(G.lse64(c)), _f32(G.lse64(u))
    out = G.combine_row(c, u, lse_c, lse_u, 3.0, G.log_beta(beta))
    lc = P.bf16_float(c).astype(np.float64)
    keep = G.kept_by_floor(c, beta)
    assert keep[np.argmax(lc)], "the maximum column survives"
    if beta == 0.0:
        assert keep.all() and np.array_equal(out, G.combine_row(c, u, lse_c, lse_u, 3.0)), "beta = 0 is off"
    else:
        # exactly the columns whose probability is below beta times the top one's, up to the fp32 rounding of the threshold
        p = np.exp(lc - lc.max())
        clear = np.abs(p / beta - 1) > 1e-5
        assert np.array_equal(keep[clear], (p >= beta)[clear])
        assert 0 < keep.sum() < V
    assert np.array_equal(out == G.NINF, ~keep), "dropped columns are -inf, kept ones are not"


def test_keyword_surface():
    from unimedvl_amd import ops
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.guidance import GuidedDecodeSession
    from unimedvl_amd.interactive_vqa_inferencer import DEFAULT_CONFIG
    sig = inspect.signature(Bagel.generate_text).parameters
    for name, default in (("guidance_scale", 1.0), ("guidance_past_key_values", None), ("guidance_query_position_ids", None),
                          ("guidance_plausibility", 0.0)):
        assert sig[name].default == default and sig[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    sig = inspect.signature(Bagel.chat).parameters
    for name, default in (("guidance_scale", 1.0), ("negative_prompt", None), ("guidance_plausibility", 0.0)):
        assert sig[name].default == default and sig[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert DEFAULT_CONFIG[name] == default
    assert issubclass(GuidedDecodeSession, __import__("unimedvl_amd.decode", fromlist=["DecodeSession"]).DecodeSession)
    assert ops.check_guidance() == (1.0, 0.0) and ops.check_guidance(3, 0.1) == (3.0, 0.1)
    assert ops.check_guidance(0.0) == (0.0, 0.0)
    for bad in (-0.5, float("nan"), float("inf"), "3", True, None):
        with pytest.raises(ValueError):
            ops.check_guidance(bad)
    for bad in (-0.1, 1.0, 1.5, float("nan"), "0.1"):
        with pytest.raises(ValueError):
            ops.check_guidance(2.0, bad)
    with pytest.raises(ValueError):
        ops.check_guidance(1.0, 0.1)                         # a floor without guidance
    with pytest.raises(TypeError):
        ops.check_guidance(2.0, 0.0, no_such_keyword=1)


REFUSED = [dict(num_beams=2), dict(draft_len=2), dict(sampling=object()), dict(row_sampling=[object()]), dict(repetition_penalty=1.2),
           dict(presence_penalty=0.5), dict(frequency_penalty=0.5), dict(logit_bias={3: 1.0}), dict(no_repeat_ngram_size=2),
           dict(no_repeat_ngram_size=[0, 2]), dict(constraint=object()), dict(choices=["yes", "no"]), dict(bad_words_ids=[[1, 2]]),
           dict(bad_words=["no"]), dict(suppress_tokens=[4]), dict(begin_suppress_tokens=[4]), dict(min_new_tokens=3),
           dict(forced_ids=torch.zeros((2, 2), dtype=torch.int64)), dict(return_logits=True)]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: next(iter(kw)))
def test_refusals_need_no_launch(kw):
    from unimedvl_amd import ops
    with pytest.raises(ValueError, match=next(iter(kw))):
        ops.check_guidance(3.0, 0.0, **kw)
    assert ops.check_guidance(1.0, 0.0, **kw) == (1.0, 0.0), "with guidance off the keyword is someone else's"


def test_neutral_keywords_pass_and_the_unfused_step_is_refused(monkeypatch):
    from unimedvl_amd import ops
    off = dict(ops.GUIDANCE_EXCLUDES)
    off.update(bad_words_ids=[], min_new_tokens=[0, 0], no_repeat_ngram_size=[0, 0], logit_bias={})
    assert ops.check_guidance(3.0, 0.5, **off) == (3.0, 0.5)
    monkeypatch.setenv("UMV_DECODE_FUSED_ARGMAX", "0")
    with pytest.raises(ValueError, match="UMV_DECODE_FUSED_ARGMAX"):
        ops.check_guidance(3.0)
    assert ops.check_guidance(1.0) == (1.0, 0.0)


def test_pair_tables():
    from unimedvl_amd import ops
    assert ops.check_guidance_pairs([3, 4, 5, -1, -1, -1]) == [3, 4, 5, -1, -1, -1]
    assert ops.check_guidance_pairs(torch.tensor([-1, -1], dtype=torch.int32)) == [-1, -1]
    for bad in ([1, 0], [1, 2, -1], [2, 2, -1], [0, -1], [5, -1], [-2, -1]):      # a cycle, a chain, a shared row, itself, outside
        with pytest.raises(ValueError):
            ops.check_guidance_pairs(bad)
        # ... and what the kernels do with such a table: no row is both written and read, no row is fed twice
        M = len(bad)
        act = [G.partner(bad, [3.0] * M, c) for c in range(M)]
        us = [u for u in act if u >= 0]
        assert len(us) == len(set(us)) and not set(us) & {c for c, u in enumerate(act) if u >= 0}
    with pytest.raises(ValueError):
        ops.check_guidance_pairs([1, -1], rows=3)


def test_documents_name_the_keywords():
    for doc, words in (("README.md", ("guidance_scale", "negative_prompt", "guidance_plausibility", "guidance_past_key_values")),
                       ("DESIGN.md", ("guidance_scale", "guidance_plausibility", "logit_guidance.hip", "umv_guidance_feed"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, f"{doc} does not name {w}"
    header = open(os.path.join(ROOT, "include", "unimedvl_hip.h")).read()
    assert "classifier-free guidance for text" in header and "umv_logit_guidance_bf16" in header


def test_log_beta_is_computed_once_on_the_host():
    assert G.log_beta(0.0) == -np.inf and G.log_beta(0.1) == np.float32(math.log(0.1))
