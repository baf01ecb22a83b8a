"""Logit penalties without a GPU: the numpy model of the definition (tests/penalty_ref.py) against a straight torch restatement on the
edge cases, the argument checks of ops.check_penalties, the C ABI of umv_logit_penalty_bf16 (header, ctypes mirror, _SIGS) and the
keywords on the public interface."""
import ctypes
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import penalty_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unimedvl_hip.h")
BF16 = torch.bfloat16


def _torch_adjust(logits, count, in_context, bias, r, presence, frequency):
    """the definition on torch tensors: logits bf16 [V], count int [V], in_context bool [V], bias fp32 [V] -> bf16 [V]"""
    a = logits.float()
    seen = (count > 0) | in_context
    if r != 1.0:
        rr = torch.tensor(r, dtype=torch.float32)
        a = torch.where(seen, torch.where(a < 0, a * rr, a / rr), a)
    pen = torch.tensor(presence, dtype=torch.float32) + torch.tensor(frequency, dtype=torch.float32) * count.float()
    a = torch.where(count > 0, a - pen, a)
    a = torch.where(bias != 0, a + bias, a)
    return a.to(BF16)


def _bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("r", [1.0, 1.3, 0.8])
@pytest.mark.parametrize("presence,frequency", [(0.0, 0.0), (0.5, 0.25), (-0.75, 0.1)])
def test_model_equals_a_torch_restatement(r, presence, frequency):
    V = 330
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn(V, generator=g) * 3).to(BF16)
    special = {1: 0.0, 2: -0.0, 5: -0.0, 6: float("-inf"), 7: float("nan"), 8: -3.0, 9: 0.0, 40: 3.0e38, 41: -3.0e38, 42: 1e-40}
    for n, v in special.items():
        logits[n] = v
    context = [1, 2, 20, 40, 42, 300]
    bias = {20: 1.5, 100: -2.25, 101: float("-inf"), 6: 4.0, 329: 0.0}
    h = P.History(V, cap=64, context=context, bias=bias)
    gen = [0, 5, 6, 7, 8, 9, 9, 9, 20, 41, 200, 200, 329]          # the first is the start token: not counted
    for t in gen:
        h.record(t)
    assert h.len == h.n_static + len(set(gen[1:]) - set(context) - set(bias)) and len(set(h.list[:h.len].tolist())) == h.len
    count = torch.zeros(V, dtype=torch.int64)
    for t in gen[1:]:
        count[t] += 1
    assert np.array_equal(h.count & P.COUNT_MASK, count.numpy().astype(np.uint32))
    ctx = torch.zeros(V, dtype=torch.bool)
    ctx[context] = True
    b = torch.zeros(V, dtype=torch.float32)
    for n, v in bias.items():
        b[n] = v
    want = _bits(_torch_adjust(logits, count, ctx, b, r, presence, frequency))
    got = P.adjust_row(_bits(logits), h, r, presence, frequency)
    bad = np.flatnonzero(~P.same_bits(got, want))
    assert bad.size == 0, (bad, got[bad], want[bad])
    untouched = np.ones(V, dtype=bool)
    untouched[[n for _, n in h.entries()]] = False
    assert np.array_equal(got[untouched], _bits(logits)[untouched]), "a column that is neither seen nor biased keeps its bits"
    assert math.isnan(float(P.bf16_float(got[7:8])[0])) and P.bf16_float(got[6:7])[0] == -np.inf and P.bf16_float(got[101:102])[0] == -np.inf
    if r == 1.0 and presence == 0.0 and frequency == 0.0:
        assert np.array_equal(got[[1, 2, 5, 9, 329]], _bits(logits)[[1, 2, 5, 9, 329]]), "neutral parameters keep -0 and +0"


def test_bf16_rounding_and_keys_of_the_model():
    x = torch.tensor([1.00390625, 1.01171875, -1.00390625, 3.0e38, 3.4e38, 1e-40, 0.0, -0.0, float("inf")], dtype=torch.float32)
    assert np.array_equal(P.bf16_bits(x.numpy()), _bits(x.to(BF16)))
    g = torch.Generator().manual_seed(9)
    row = (torch.randn(40, generator=g) * 2).to(BF16)
    row[3] = row[19] = row[:32].max()                   # a tie inside tile 0 / across tiles: the lowest column wins
    row[35] = float("nan")
    row[36] = -0.0
    keys = P.greedy_keys(_bits(row))
    cols = (0xFFFFFFFF - (keys & 0xFFFFFFFF)).astype(np.int64)
    assert cols.tolist() == [3, 19, 35]
    m, s = P.tile_stats(_bits(torch.full((40,), float("-inf")).to(BF16)))
    assert np.isneginf(m).all() and (s == 0).all()
    m, s = P.tile_stats(_bits(row[:32]), 0.7)
    y = (row[:32].float() / torch.tensor(0.7)).to(BF16).double().reshape(2, 16)
    assert np.array_equal(m, y.max(-1).values.numpy()) and np.allclose(s, torch.exp(y - y.max(-1, keepdim=True).values).sum(-1).numpy(), rtol=1e-12)


def test_check_penalties():
    from unimedvl_amd import ops
    assert ops.check_penalties() == (1.0, 0.0, 0.0, {})
    assert ops.check_penalties(1.2, 0.5, -0.25, {7: -math.inf, 9: 2}, vocab=10) == (1.2, 0.5, -0.25, {7: -math.inf, 9: 2.0})
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=math.inf),
                dict(repetition_penalty=math.nan), dict(repetition_penalty="1.1"), dict(repetition_penalty=True),
                dict(presence_penalty=math.inf), dict(presence_penalty=None), dict(frequency_penalty=math.nan),
                dict(logit_bias=[(1, 2.0)]), dict(logit_bias={-1: 1.0}), dict(logit_bias={1.5: 1.0}), dict(logit_bias={True: 1.0}),
                dict(logit_bias={3: math.nan}), dict(logit_bias={3: "x"}), dict(logit_bias={10: 1.0}, vocab=10)):
        with pytest.raises(ValueError):
            ops.check_penalties(**bad)


def test_the_entry_point_is_bound_and_documented():
    from unimedvl_amd import _lib
    assert "umv_logit_penalty_bf16" in _lib._SIGS
    res, args = _lib._SIGS["umv_logit_penalty_bf16"]
    assert res is ctypes.c_int and len(args) == 2 and args[0]._type_ is _lib.LogitPenaltyArgs
    assert (_lib.PENALTY_COUNT_MASK, _lib.PENALTY_CONTEXT, _lib.PENALTY_LISTED) == (P.COUNT_MASK, P.CONTEXT, P.LISTED)
    text = open(HEADER).read()
    sec = text[text.index("logit penalties and bias"):text.index("int umv_logit_penalty_bf16")]
    for word in ("repetition_penalty", "presence", "frequency", "bias", "ADJUSTED, untruncated softmax", "before temperature",
                 "bf16_round_nearest_even", "NaN stays NaN", "keeps its bits", "cap", "FRESH", "UMV_ERR_ARG", "argmax_partial = NULL"):
        assert word in sec, word
    for name, value in (("UMV_PENALTY_COUNT_MASK", P.COUNT_MASK), ("UMV_PENALTY_CONTEXT", P.CONTEXT), ("UMV_PENALTY_LISTED", P.LISTED)):
        assert int(re.search(rf"#define {name} (0x[0-9A-Fa-f]+)u", text).group(1), 16) == value
    from unimedvl_amd import build
    assert "logit_penalty.hip" in build.SOURCES


def test_ctypes_mirror_has_the_layout_of_the_header(tmp_path):
    from unimedvl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct\s*\{([^{}]*)\}\s*umv_logit_penalty_args\s*;", src).group(1)
    fields = [re.findall(r"[A-Za-z_][A-Za-z_0-9]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert fields == [n for n, _ in _lib.LogitPenaltyArgs._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(umv_logit_penalty_args));']
    lines += [f'  printf("{f} %zu\\n", offsetof(umv_logit_penalty_args, {f}));' for f in fields] + ["  return 0;", "}"]
    (tmp_path / "abi.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-o", str(tmp_path / "abi"), str(tmp_path / "abi.c")])
    c = dict(ln.split() for ln in subprocess.check_output([str(tmp_path / "abi")], text=True).splitlines())
    assert ctypes.sizeof(_lib.LogitPenaltyArgs) == int(c["size"])
    for f in fields:
        assert getattr(_lib.LogitPenaltyArgs, f).offset == int(c[f]), f


PENALTY_KW = ("repetition_penalty", "presence_penalty", "frequency_penalty", "logit_bias")


def test_the_public_interface_carries_the_keywords():
    from unimedvl_amd import bagel, decode, inferencer, serving
    sig = inspect.signature(decode.DecodeSession.__init__).parameters
    for k in PENALTY_KW + ("penalty_context_ids",):
        assert k in sig, k
    assert (sig["repetition_penalty"].default, sig["presence_penalty"].default, sig["frequency_penalty"].default,
            sig["logit_bias"].default, sig["penalty_context_ids"].default) == (1.0, 0.0, 0.0, None, None)
    assert "penalty_context_ids" in inspect.signature(decode.DecodeSession.set_slot).parameters
    for fn in (bagel.Bagel.generate_text, bagel.Bagel.chat, inferencer.InterleaveInferencer.gen_text,
               inferencer.InterleaveInferencer.gen_text_batch, serving.ContinuousBatcher.__init__):
        p = inspect.signature(fn).parameters
        for k in PENALTY_KW:
            assert k in p and p[k].default == sig[k].default, (fn.__qualname__, k)
            assert p[k].kind is inspect.Parameter.KEYWORD_ONLY, (fn.__qualname__, k)      # never bound by a positional truncation argument
    for fn in (bagel.Bagel.chat, serving.ContinuousBatcher.__init__):
        assert inspect.signature(fn).parameters["penalize_prompt"].default is False
    # the pipelines carry them as text_* next to text_top_k, with gen_text's defaults, and hand them on under gen_text's names
    for fn in (inferencer.InterleaveInferencer.interleave_inference, inferencer.InterleaveInferencer.interleave_inference_for_vqa_reconstruction_ver1,
               inferencer.InterleaveInferencer.interleave_inference_for_vqa_reconstruction_ver0_1,
               inferencer.InterleaveInferencer.interleave_inference_for_vqa_reconstruction_ver0,
               inferencer.InterleaveInferencer.batch_interleave_inference):
        p = inspect.signature(fn).parameters
        for k in PENALTY_KW:
            assert p["text_" + k].default == sig[k].default and p["text_" + k].kind is inspect.Parameter.KEYWORD_ONLY, (fn.__qualname__, k)
        src = inspect.getsource(fn)
        assert "_penalties(text_repetition_penalty, text_presence_penalty, text_frequency_penalty, text_logit_bias)" in src or \
            all(f"{k}=text_{k}" in src for k in PENALTY_KW), fn.__qualname__
    assert inferencer._penalties(1.1, 0.2, 0.3, {4: 1.0}) == dict(repetition_penalty=1.1, presence_penalty=0.2, frequency_penalty=0.3,
                                                                 logit_bias={4: 1.0})
    assert set(inspect.signature(inferencer.InterleaveInferencer.gen_text).parameters) >= set(inferencer._penalties(1, 0, 0, None))
    # VQAInferencer: config keys with neutral defaults, per-call overrides whose None means "the config's value"
    from unimedvl_amd import interactive_vqa_inferencer as vqa
    neutral = dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None, penalize_prompt=False)
    assert {k: vqa.DEFAULT_CONFIG[k] for k in neutral} == neutral
    p = inspect.signature(vqa.VQAInferencer.infer_single).parameters
    assert all(p[k].default is None and p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in neutral)
    assert set(inspect.signature(bagel.Bagel.chat).parameters) >= set(neutral)
