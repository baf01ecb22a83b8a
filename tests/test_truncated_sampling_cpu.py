"""Truncated sampling (top-k / top-p / min-p), the parts that need no GPU: the tests' fp64 reference (tests/truncation_ref.py) against
torch on tie-free rows and on rows with ties, the ABI and the sanitizer driver carry the two entries, the public keywords exist with
their defaults off, and a bad value raises."""
import inspect
import math
import os
import re

import pytest
import torch

import truncation_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16


def _tie_free_row(V, seed):
    """V distinct bf16 values in about [-8, 8], shuffled: at T = 1 every class is one column"""
    g = torch.Generator().manual_seed(seed)
    pool = torch.unique((torch.randn(8 * V, generator=g) * 3).to(BF16).float())
    pool = pool[pool != 0]
    return pool[torch.randperm(pool.numel(), generator=g)[:V]].to(BF16)


@pytest.mark.parametrize("V", [40, 70, 320])
def test_reference_matches_torch_on_tie_free_rows(V):
    logits = _tie_free_row(V, V)
    y = R.pick_value(logits, 1.0)
    row = R.classes(y)
    assert len(row.vals) == V and int(row.cnt.max()) == 1
    p = torch.softmax(y, -1)
    srt = torch.sort(p, descending=True).values
    for k in (1, 5, V - 1, V, V + 3):
        i, cut, n = R.cutoff(row, top_k=k)
        kk = min(k, V)
        assert n == kk and cut == float(torch.topk(y, kk).values[-1])
    for tp in (0.1, 0.5, 0.9, 0.999):
        i, cut, n = R.cutoff(row, top_p=tp)
        want = int((srt.cumsum(0) >= R._f32(tp)).nonzero()[0]) + 1          # descending sort plus cumsum: the smallest prefix reaching top_p
        assert n == want and cut == float(torch.sort(y, descending=True).values[want - 1])
        assert R.band(row, top_p=tp)[0] <= i <= R.band(row, top_p=tp)[1]
    for mp in (0.5, 0.05, 1e-4):
        i, cut, n = R.cutoff(row, min_p=mp)
        assert n == int((p / p.max() >= R._f32(mp)).sum())                  # the probability ratio
    # sequential: top_p works on what top_k kept
    i, cut, n = R.cutoff(row, top_k=10, top_p=0.9)
    top = torch.sort(y, descending=True).values[:10]
    q = torch.softmax(top, -1).cumsum(0)
    assert n == int((q >= R._f32(0.9)).nonzero()[0]) + 1
    assert R.cutoff(row, top_k=10, top_p=0.9, min_p=0.05)[2] == min(n, R.cutoff(row, min_p=0.05)[2])


def test_reference_keeps_whole_classes_on_tied_rows():
    # logits on a 0.5 grid: 3 (x2), 2.5 (x3), 2 (x1), 1.5 (x4), then a tail; a tie straddles k = 4
    logits = torch.tensor([1.5, 3.0, 2.5, 1.5, 2.5, 2.0, 3.0, 1.5, 2.5, 1.5] + [0.5 * (i % 5) - 3 for i in range(30)]).to(BF16)
    y = R.pick_value(logits, 1.0)
    row = R.classes(y)
    assert row.vals[:4].tolist() == [3.0, 2.5, 2.0, 1.5] and row.cnt[:4].tolist() == [2, 3, 1, 4]
    assert R.cutoff(row, top_k=4)[1:] == (2.5, 5)                           # the k-th value is 2.5: all three 2.5s stay
    assert R.cutoff(row, top_k=2)[1:] == (3.0, 2) and R.cutoff(row, top_k=1)[1:] == (3.0, 2)
    assert R.cutoff(row, top_k=6)[1:] == (2.0, 6) and R.cutoff(row, top_k=7)[1:] == (1.5, 10)
    z = float(row.mass.sum())
    want = 2 + 3 * math.exp(-0.5)                                           # mass of the two top classes about M = 3
    assert abs(float(row.cum[1]) - want) < 1e-12
    tp = (want / z) - 1e-3                                                  # just inside the second class
    assert R.cutoff(row, top_p=tp)[1:] == (2.5, 5)
    assert R.cutoff(row, top_p=(want / z) + 1e-3)[1:] == (2.0, 6)
    assert R.cutoff(row, min_p=math.exp(-1.25))[1:] == (2.0, 6)            # y - M >= -1.25: 3, 2.5, 2
    # T = 0.3: the rounding of logit / T to bf16 merges values that differ as logits
    fine = torch.tensor([1.0 + i / 128 for i in range(128)]).to(BF16)      # 128 distinct bf16 logits, every value of [1, 2)
    assert len(torch.unique(fine.float())) == 128
    y3 = R.pick_value(fine, 0.3)
    r3 = R.classes(y3)
    assert len(r3.vals) < 128 and int(r3.cnt.sum()) == 128
    for k in (1, 3, 10):
        i, cut, n = R.cutoff(r3, top_k=k)
        assert n >= k and n == int((y3 >= cut).sum()) and int((y3 > cut).sum()) < k
    # -0 and +0 are one class; NaN is the top class and takes all; a row of -inf is one class
    z0 = R.classes(torch.tensor([0.0, -0.0, 1.0], dtype=torch.float64))
    assert z0.cnt.tolist() == [1, 2]
    nn = R.classes(torch.tensor([float("nan"), 5.0, float("nan"), 1.0], dtype=torch.float64))
    assert nn.has_nan and R.cutoff(nn, top_p=0.5)[2] == 2 and math.isnan(R.cutoff(nn, top_k=3)[1]) and R.band(nn, top_k=3) == (0, 0)
    ninf = R.classes(torch.full((7,), float("-inf"), dtype=torch.float64))
    assert R.cutoff(ninf, top_k=2, top_p=0.5, min_p=0.1)[1:] == (float("-inf"), 7)


def test_header_binding_and_driver_carry_both_entries():
    from unimedvl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "unimedvl_hip.h")).read(), flags=re.S)
    drv = open(os.path.join(ROOT, "tools", "abi_sanitize_driver.cpp")).read()
    for name in ("umv_sample_truncated_bf16", "umv_decode_step_end_truncated"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in _lib._SIGS, name
        assert re.search(r"EXPECT_ERR\(" + name + r"\(nullptr", drv), name     # NULL arguments
        assert len(re.findall(name + r"\(", drv)) >= 3, name                    # and invalid ones
    assert len(_lib._SIGS["umv_sample_truncated_bf16"][1]) == 14
    assert len(_lib._SIGS["umv_decode_step_end_truncated"][1]) == len(_lib._SIGS["umv_decode_step_end_logprob"][1]) + 6
    assert len(_lib._SIGS["umv_decode_step_end_logprob"][1]) == 19 and len(_lib._SIGS["umv_sample_bf16"][1]) == 9   # the old entries keep theirs
    fields = [n for n, _ in _lib.GemmArgs._fields_]
    assert fields[-1] == "lse_partial"                                          # no GEMM struct change


OFF = dict(top_k=0, top_p=1.0, min_p=0.0)


def _last_three_off(fn, names=("top_k", "top_p", "min_p")):
    p = inspect.signature(fn).parameters
    assert list(p)[-3:] == list(names), (fn.__qualname__, list(p)[-3:])         # the new keywords come last
    assert [p[n].default for n in names] == [0, 1.0, 0.0], fn.__qualname__


def test_public_keywords_exist_and_default_off():
    from unimedvl_amd import ops
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.decode import DecodeSession
    from unimedvl_amd.inferencer import InterleaveInferencer
    from unimedvl_amd.interactive_vqa_inferencer import DEFAULT_CONFIG, VQAInferencer
    from unimedvl_amd.serving import ContinuousBatcher
    for fn in (DecodeSession.__init__, Bagel.generate_text, Bagel.chat, InterleaveInferencer.gen_text, InterleaveInferencer.gen_text_batch,
               ContinuousBatcher.__init__):
        _last_three_off(fn)
    text = ("text_top_k", "text_top_p", "text_min_p")
    for fn in (InterleaveInferencer.interleave_inference, InterleaveInferencer.interleave_inference_for_vqa_reconstruction_ver1,
               InterleaveInferencer.interleave_inference_for_vqa_reconstruction_ver0_1,
               InterleaveInferencer.interleave_inference_for_vqa_reconstruction_ver0, InterleaveInferencer.batch_interleave_inference):
        _last_three_off(fn, text)
        assert "text_temperature" in inspect.signature(fn).parameters
    assert {k: DEFAULT_CONFIG[k] for k in OFF} == OFF
    p = inspect.signature(VQAInferencer.infer_single).parameters
    assert list(p)[-3:] == ["top_k", "top_p", "min_p"] and all(p[k].default is None for k in OFF)       # None = the config's value
    s = inspect.signature(ops.sample_truncated).parameters
    assert list(s)[:4] == ["logits", "temperature", "seed", "step"] and [s[k].default for k in OFF] == [0, 1.0, 0.0]
    assert s["cut_y"].default is None and s["n_kept"].default is None
    e = inspect.signature(ops.decode_step_end_truncated).parameters
    assert [e[k].default for k in OFF] == [0, 1.0, 0.0] and e["cut_y"].default is None and e["forced_ids"].default is None


@pytest.mark.parametrize("bad", [dict(top_k=-1), dict(top_k=2.5), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")),
                                 dict(min_p=-0.1), dict(min_p=1.0), dict(min_p=float("nan"))])
def test_a_bad_value_raises(bad):
    from unimedvl_amd import ops
    from unimedvl_amd.serving import ContinuousBatcher
    with pytest.raises(ValueError, match=next(iter(bad))):
        ops.check_truncation(**dict(OFF, **bad))
    with pytest.raises(ValueError, match=next(iter(bad))):     # before anything touches a device
        ContinuousBatcher(None, None, None, None, do_sample=True, **bad)
    assert ops.check_truncation(50, 0.9, 0.05) == (50, 0.9, 0.05) and ops.check_truncation(**OFF) == (0, 1.0, 0.0)


def test_filters_need_do_sample():
    from unimedvl_amd.serving import ContinuousBatcher
    with pytest.raises(ValueError, match="do_sample"):
        ContinuousBatcher(None, None, None, None, top_k=5)
