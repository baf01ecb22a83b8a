"""Token log-probabilities, the parts that need no GPU: the ABI carries the new entry points and field (the generic ABI tests then
check layout and signatures), the sanitizer driver calls them, the tests' fp64 reference is torch's log_softmax, and the public
keywords exist with their defaults off."""
import inspect
import os
import re

import torch

import logprob_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_carry_the_new_entry_points():
    from unimedvl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "unimedvl_hip.h")).read(), flags=re.S)
    for name in ("umv_decode_step_end_logprob", "umv_token_logprob_bf16"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in _lib._SIGS, name
    assert re.search(r"float\s*\*\s*lse_partial\s*;", src)
    fields = [n for n, _ in _lib.GemmArgs._fields_]
    assert fields[-1] == "lse_partial" and "argmax_partial" in fields          # appended: every older field keeps its offset
    n = len(_lib._SIGS["umv_decode_step_end_argmax"][1])
    assert n == 12                                                              # the old entry keeps its signature


def test_sanitizer_driver_calls_both_entry_points():
    drv = open(os.path.join(ROOT, "tools", "abi_sanitize_driver.cpp")).read()
    for name in ("umv_decode_step_end_logprob", "umv_token_logprob_bf16"):
        assert re.search(r"EXPECT_ERR\(" + name + r"\(nullptr", drv), name     # NULL arguments
        assert len(re.findall(name + r"\(", drv)) >= 2, name                    # and invalid ones
    assert "lse_partial" in drv


def test_reference_is_log_softmax_in_fp64():
    g = torch.Generator().manual_seed(7)
    logits = (torch.randn(5, 70, generator=g) * 4).to(torch.bfloat16)
    logits[:, 32:48] = float("-inf")           # a whole tile
    logits[:, 20:23] = float("-inf")           # part of one
    ids = torch.tensor([0, 5, 69, 31, 48])
    for T in (0.0, 0.7, 1.0, 2.5):
        y = logits.double() if T == 0 else (logits.float() / T).to(torch.bfloat16).double()
        want = torch.log_softmax(y, -1).gather(1, ids[:, None])[:, 0]
        got = R.logprob(logits, ids, T)
        assert got.dtype == torch.float64 and torch.isfinite(got).all()
        assert (got - want).abs().max() < 1e-12, T
        m, s = R.tile_stats(logits, T)
        assert m.shape == (5, 5) and (m[:, 2] == float("-inf")).all() and (s[:, 2] == 0).all() and not torch.isnan(s).any()
        assert torch.equal(m[:, 4], y[:, 64:70].max(-1).values)                 # the last tile holds 6 columns
        lse = torch.log((s * torch.exp(m - m.max(-1, keepdim=True).values)).sum(-1)) + m.max(-1).values
        assert (lse - torch.logsumexp(y, -1)).abs().max() < 1e-12               # the tiles merge to the row's logsumexp
    # the rounding of logits / T is part of the definition: without it the value differs
    y_unrounded = logits.double() / 0.7
    assert (torch.log_softmax(y_unrounded, -1)[0, 0] - R.logprob(logits, ids, 0.7)[0]).abs() > 1e-6
    bad = logits.clone()
    bad[1, 3] = float("nan")
    got = R.logprob(bad, ids)
    assert torch.isnan(got[1]) and torch.isfinite(got[[0, 2, 3, 4]]).all()


def test_public_keywords_exist_and_default_off():
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.decode import DecodeSession
    from unimedvl_amd.interactive_vqa_inferencer import DEFAULT_CONFIG, VQAInferencer
    from unimedvl_amd.serving import ContinuousBatcher
    assert inspect.signature(ContinuousBatcher.__init__).parameters["logprobs"].default is False
    assert inspect.signature(Bagel.generate_text).parameters["return_logprobs"].default is False
    p = inspect.signature(DecodeSession.__init__).parameters
    assert p["logprobs"].default is False and p["forced_ids"].default is None
    sc = inspect.signature(Bagel.score).parameters
    assert list(sc)[1:] == ["tokenizer", "new_token_ids", "image_transform", "images", "prompt", "candidates", "append_eos"]
    assert sc["append_eos"].default is True
    assert list(inspect.signature(VQAInferencer.score).parameters)[1:4] == ["image", "question", "candidates"]
    assert "return_logprobs" not in DEFAULT_CONFIG                               # off unless asked for
    from unimedvl_amd import ops
    g = inspect.signature(ops.gemm).parameters
    assert g["lse_partial"].default is None and g["lse_partial"].kind is inspect.Parameter.KEYWORD_ONLY
    t = inspect.signature(ops.token_logprob).parameters
    assert list(t) == ["logits", "ids", "temperature", "out"] and t["temperature"].default == 0.0 and t["out"].default is None
    assert callable(ops.decode_step_end_logprob)
