"""no_repeat_ngram_size without a GPU: the plain-Python definition (tests/ngram_ref.py) against a second implementation and against
transformers' NoRepeatNGramLogitsProcessor, its edge cases, the value check of ops.check_ngram, the C ABI of umv_logit_ngram_ban_bf16
(header, ctypes mirror, _SIGS, driver), the keywords on the public interface, and - behind the recorder of tests/abi_recorder.py -
the one extra call a step issues with the keyword on."""
import ctypes
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ngram_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unimedvl_hip.h")
V = 4         # the alphabet of the random histories: small, so that n-grams repeat


def _random_histories(count, seed, dirty=False):
    """(history, n) pairs: lengths 0..24 over a 4-letter alphabet, n = 1..5; dirty: with separators and out-of-range entries mixed in"""
    rng = np.random.default_rng(seed)
    for _ in range(count):
        L = int(rng.integers(0, 25))
        h = rng.integers(0, V, L).tolist()
        if dirty:
            h = [t if rng.random() > 0.15 else int(rng.choice([-1, V, V + 3, -7])) for t in h]
        yield h, int(rng.integers(1, 6))


# ----------------------------------------------------------------------------- the definition
def test_reference_equals_a_second_implementation():
    banning = 0
    for dirty in (False, True):
        for h, n in _random_histories(2000, 11 + dirty, dirty):
            a, b = R.banned(h, n, V), R.banned_table(h, n, V)
            assert a == b, (h, n, a, b)
            banning += bool(a)
    assert banning > 1000, "the random histories must ban on a good share of the rows"


def test_reference_equals_transformers_processor():
    pytest.importorskip("transformers")
    from transformers import NoRepeatNGramLogitsProcessor
    banning = mismatches = 0
    for h, n in _random_histories(2000, 5):
        if not h:
            continue            # (the processor is never called on an empty sequence: a step is always fed a token)
        scores = NoRepeatNGramLogitsProcessor(n)(torch.tensor([h], dtype=torch.long), torch.zeros((1, V)))
        hf = torch.isinf(scores[0]).nonzero().flatten().tolist()
        ours = R.banned(h, n, V)
        mismatches += hf != ours
        banning += bool(ours)
    assert mismatches == 0 and banning > 500, (mismatches, banning)


def test_edge_cases_of_the_definition():
    a, b, c = 0, 1, 2
    assert R.banned([a, a], 2, V) == [a], "the candidate that overlaps the suffix counts"
    assert R.banned([a, b, a], 3, V) == [] and R.banned([a, b], 3, V) == [], "L < n, and L = n without a repeat"
    assert R.banned([a, a, a], 3, V) == [a]
    assert R.banned([a, b, c, a, b], 3, V) == [c]
    assert R.banned([c, a, -1, b, 9], 1, V) == [a, b, c], "n = 1 bans every history token inside the vocabulary"
    assert R.banned([a, b, c, -1, a, b], 3, V) == [c], "a separator between the n-grams is harmless"
    assert R.banned([a, -1, c, a, -1], 3, V) == [], "a separator in the suffix never matches, equal integers or not"
    assert R.banned([a, 7, c, a, 7], 3, V) == [], "nor does an out-of-range id"
    assert R.banned([a, b, 7, a, b], 3, V) == [] and R.banned([a, b, -1, a, b], 3, V) == [], "a follower outside [0, V) is not banned"
    assert R.banned([a, b, c, a, b], 0, V) == [] and R.banned([a] * 40, 17, V) == [] and R.banned([a, a], -1, V) == []
    assert R.banned([a] * 40, 16, V) == [a]
    bits = np.array([0x3F80, 0x7FC0, 0xFF80, 0xC000], dtype=np.uint16)
    out, cols = R.ban_row(bits, [1, 2, 0, 3, 1], 1)
    assert cols == [0, 1, 2, 3] and (out == R.NINF).all(), "NaN and -inf columns become / stay -inf"
    out, cols = R.ban_row(bits, [0, 1, 0], 2)
    assert cols == [1] and out.tolist() == [0x3F80, R.NINF, 0xFF80, 0xC000] and bits[1] == 0x7FC0, "every other column keeps its bits"


def test_history_record():
    h = R.History(4, [5, -1])
    h.record(7)
    h.record(1 << 31)                   # no column: recorded as a separator
    assert h.tokens() == [5, -1, 7, -1] and h.len == 4
    h.record(9)                         # full at record time
    assert h.len == R.FULL and h.hist.tolist() == [5, -1, 7, -1]
    h.record(9)
    assert h.len == R.FULL and h.tokens() == []
    off = R.History(4, [1, 2], length=-1)
    off.record(3)
    assert off.len == -1 and off.hist.tolist() == [1, 2, 0, 0]
    bits = np.array([1, 2, 3, 4], dtype=np.uint16)
    out, cols = R.step(bits, off, 1, 1)
    assert cols == [] and np.array_equal(out, bits)
    h = R.History(3, [-5])
    h.record(-(1 << 40))
    assert h.tokens() == [-5, -1]


# ----------------------------------------------------------------------------- the value check
def test_check_ngram():
    from unimedvl_amd import _lib, ops
    assert ops.NGRAM_MAX == _lib.NGRAM_MAX == R.NGRAM_MAX == 16 and _lib.NGRAM_FULL == R.FULL
    assert [ops.check_ngram(v) for v in (0, 1, 16, 3.0)] == [0, 1, 16, 3]
    for bad in (-1, 17, 1.5, True, False, "2", None, [2], float("nan"), float("inf")):
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            ops.check_ngram(bad)
    from unimedvl_amd.sampling import SamplingParams, off_neutral, pack_row
    assert SamplingParams().no_repeat_ngram_size == 0 and SamplingParams(no_repeat_ngram_size=3.0).no_repeat_ngram_size == 3
    assert [f.name for f in SamplingParams.__dataclass_fields__.values()][-1] == "no_repeat_ngram_size"
    for bad in (-1, 17, True):
        with pytest.raises(ValueError):
            SamplingParams(no_repeat_ngram_size=bad)
    # not part of the packed table: the 48 bytes of a row do not depend on it
    assert pack_row(SamplingParams(no_repeat_ngram_size=5)).tobytes() == pack_row(SamplingParams()).tobytes()
    given = dict(do_sample=False, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, repetition_penalty=1.0, presence_penalty=0.0,
                 frequency_penalty=0.0)
    assert off_neutral(given) == []


# ----------------------------------------------------------------------------- the C ABI
def _header_fields(src, struct):
    body = re.search(r"typedef struct\s*\{([^{}]*)\}\s*" + struct + r"\s*;", src).group(1)
    return [re.findall(r"[A-Za-z_][A-Za-z_0-9]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]


def test_ctypes_mirror_has_the_layout_of_the_header(tmp_path):
    from unimedvl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fields = _header_fields(src, "umv_ngram_ban_args")
    assert fields == [n for n, _ in _lib.NgramBanArgs._fields_]
    assert fields == ["logits", "ld", "ids", "hist", "hist_ld", "hist_len", "row_n", "M", "V", "n", "temperature", "argmax_partial",
                      "lse_partial", "n_tiles", "seed", "step", "rows"]
    pinned = {"umv_row_sampling": None, "umv_gemm_args": None, "umv_logit_penalty_args": None}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(umv_ngram_ban_args));']
    lines += [f'  printf("{f} %zu\\n", offsetof(umv_ngram_ban_args, {f}));' for f in fields]
    lines += [f'  printf("{s} %zu\\n", sizeof({s}));' for s in pinned] + ["  return 0;", "}"]
    (tmp_path / "abi.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-o", str(tmp_path / "abi"), str(tmp_path / "abi.c")])
    c = dict(ln.split() for ln in subprocess.check_output([str(tmp_path / "abi")], text=True).splitlines())
    assert ctypes.sizeof(_lib.NgramBanArgs) == int(c["size"])
    for f in fields:
        assert getattr(_lib.NgramBanArgs, f).offset == int(c[f]), f
    # the structures the issue leaves alone: the per-row size travels in an array of its own
    assert int(c["umv_row_sampling"]) == 48 == ctypes.sizeof(_lib.RowSampling)
    assert int(c["umv_gemm_args"]) == ctypes.sizeof(_lib.GemmArgs) and int(c["umv_logit_penalty_args"]) == ctypes.sizeof(_lib.LogitPenaltyArgs)


def test_the_entry_point_is_bound_documented_and_driven():
    from unimedvl_amd import _lib, build
    res, args = _lib._SIGS["umv_logit_ngram_ban_bf16"]
    assert res is ctypes.c_int and len(args) == 2 and args[0]._type_ is _lib.NgramBanArgs and args[1] is ctypes.c_void_p
    text = open(HEADER).read()
    sec = text[text.index("no-repeat n-grams"):text.index("int umv_logit_ngram_ban_bf16")]
    for word in ("row_n", "UMV_NGRAM_MAX", "separator", "never matches", "overlaps the suffix", "0xFF80", "REPLACES", "renormalised",
                 "lm_head, [penalty], ngram ban, [constrain], step end", "UMV_NGRAM_FULL", "no byte of the row", "empty ban set",
                 "UMV_ERR_ARG", "NoRepeatNGramLogitsProcessor"):
        assert word in sec, word
    assert re.search(r"argmax_partial =\s+\*\s+NULL: record and ban only", sec)
    assert int(re.search(r"#define UMV_NGRAM_MAX (\d+)", text).group(1)) == _lib.NGRAM_MAX
    assert int(re.search(r"#define UMV_NGRAM_FULL \((-\d+)\)", text).group(1)) == _lib.NGRAM_FULL
    assert "logit_ngram.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "logit_ngram.hip"))
    drv = open(os.path.join(ROOT, "tools", "abi_sanitize_driver.cpp")).read()
    assert re.search(r"EXPECT_ERR\(umv_logit_ngram_ban_bf16\(nullptr", drv) and re.search(r"EXPECT_OK\(umv_logit_ngram_ban_bf16\(", drv)
    assert len(re.findall(r"EXPECT_ERR\(umv_logit_ngram_ban_bf16\(", drv)) >= 12
    kernel = open(os.path.join(build.CSRC, "logit_ngram.hip")).read()
    assert "penalty_tile(" in kernel and "__threadfence_block" in kernel
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "no_repeat_ngram_size" in open(os.path.join(ROOT, doc)).read(), doc


# ----------------------------------------------------------------------------- the public interface
def test_the_public_interface_carries_the_keywords():
    from unimedvl_amd import bagel, decode, inferencer, serving
    from unimedvl_amd import interactive_vqa_inferencer as vqa
    sig = inspect.signature(decode.DecodeSession.__init__).parameters
    assert [sig[k].default for k in ("no_repeat_ngram_size", "ngram_context_ids", "ngram_context_room", "ngram_history")] == [0, None, None, None]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("no_repeat_ngram_size", "ngram_context_ids", "ngram_context_room", "ngram_history"))
    assert inspect.signature(decode.DecodeSession.set_slot).parameters["ngram_context_ids"].default is None
    assert callable(decode.DecodeSession.copy_ngram_history)
    for fn in (bagel.Bagel.generate_text, bagel.Bagel.chat, inferencer.InterleaveInferencer.gen_text,
               inferencer.InterleaveInferencer.gen_text_batch, serving.ContinuousBatcher.__init__):
        p = inspect.signature(fn).parameters["no_repeat_ngram_size"]
        assert p.default == 0 and p.kind is inspect.Parameter.KEYWORD_ONLY, fn.__qualname__
    for fn in (bagel.Bagel.chat, serving.ContinuousBatcher.__init__):
        assert inspect.signature(fn).parameters["no_repeat_ngram_prompt"].default is False
        assert "HF" in fn.__doc__ and "counts the prompt" in fn.__doc__, fn.__qualname__
    for fn in (inferencer.InterleaveInferencer.interleave_inference, inferencer.InterleaveInferencer.interleave_inference_for_vqa_reconstruction_ver1,
               inferencer.InterleaveInferencer.interleave_inference_for_vqa_reconstruction_ver0_1,
               inferencer.InterleaveInferencer.interleave_inference_for_vqa_reconstruction_ver0,
               inferencer.InterleaveInferencer.batch_interleave_inference):
        p = inspect.signature(fn).parameters["text_no_repeat_ngram_size"]
        assert p.default == 0 and p.kind is inspect.Parameter.KEYWORD_ONLY, fn.__qualname__
        assert "no_repeat_ngram_size=text_no_repeat_ngram_size" in inspect.getsource(fn), fn.__qualname__
    assert vqa.DEFAULT_CONFIG["no_repeat_ngram_size"] == 0 and vqa.DEFAULT_CONFIG["no_repeat_ngram_prompt"] is False


@pytest.mark.parametrize("bad", [-1, 17, 2.5, True, "3"])
def test_the_keyword_surfaces_refuse_a_bad_value(bad):
    """before anything touches a device"""
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.sampling import SamplingParams
    from unimedvl_amd.serving import ContinuousBatcher
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        ContinuousBatcher(None, None, None, None, no_repeat_ngram_size=bad)
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        SamplingParams(no_repeat_ngram_size=bad)
    stub = SimpleNamespace(device="cpu", cfg=SimpleNamespace(vocab=320))
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        Bagel.generate_text(stub, SimpleNamespace(lens=[4]), max_length=4, no_repeat_ngram_size=bad)
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        Bagel.generate_text(stub, SimpleNamespace(lens=[4, 4]), max_length=4, no_repeat_ngram_size=[0, bad])


def test_drafts_refuse_a_size():
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.sampling import SamplingParams
    from unimedvl_amd.speculative import SpeculativeDecodeSession

    class Cache:
        lens = [4]
    for kw in (dict(no_repeat_ngram_size=2), dict(no_repeat_ngram_size=[2]), dict(ngram_context_ids=[[1]]), dict(ngram_history=8),
               dict(sampling=SamplingParams(no_repeat_ngram_size=2))):
        with pytest.raises(ValueError):
            SpeculativeDecodeSession(None, Cache(), None, None, 8, 2, **kw)
    SpeculativeDecodeSession.__init__.__doc__.index("n-gram")
    stub = SimpleNamespace(device="cpu", cfg=SimpleNamespace(vocab=320))
    for kw in (dict(no_repeat_ngram_size=2), dict(sampling=SamplingParams(no_repeat_ngram_size=2))):
        with pytest.raises(ValueError, match="draft_len"):
            Bagel.generate_text(stub, Cache(), max_length=4, draft_len=2, **kw)


# ----------------------------------------------------------------------------- the calls of a step
def _step_calls(arm, env, **over):
    """the names of the C calls one un-captured step issues, behind the recorder (no kernel runs)"""
    import test_decode_step_calls_cpu as D
    from abi_recorder import _seams
    calls = []
    with _seams(calls) as ops, D._env(env):
        sess = D._session(ops, arm, **over)
        del calls[:]
        sess.step(1)
        first = [name for name, _ in calls]
        del calls[:]
        sess.step(1)
        assert [name for name, _ in calls] == first, "a second step records the same calls"
        args = [a for name, a in calls if name == "umv_logit_ngram_ban_bf16"]
    return first, sess, args


@pytest.mark.parametrize("arm", ["greedy", "constraint sampled penalties", "rows", "greedy long UMV_DECODE_FUSED_ARGMAX=0"])
def test_a_step_issues_one_extra_call_between_penalty_and_constraint(arm):
    import test_decode_step_calls_cpu as D
    rows = arm == "rows"
    on = dict(row_sampling=[D._params(no_repeat_ngram_size=3), D._params(do_sample=True, temperature=0.7, top_p=0.9, repetition_penalty=1.2,
                                                                         seed=11, no_repeat_ngram_size=1)]) if rows else \
        dict(no_repeat_ngram_size=3, ngram_context_ids=[[4, 5, 4], [6]])
    env = D.ARMS[arm][1].get("env", {})
    off, s_off, _ = _step_calls(arm, env)
    off0, s_off0, _ = _step_calls(arm, env, no_repeat_ngram_size=0, ngram_context_ids=[[1], [2]])
    got, s_on, args = _step_calls(arm, env, **on)
    assert "umv_logit_ngram_ban_bf16" not in off and off0 == off
    for s in (s_off, s_off0):
        assert s.ng_hist is None and s.ng_len is None and s.ng_row_n is None, "off: nothing is allocated"
    at = got.index("umv_logit_ngram_ban_bf16")
    assert got[:at] + got[at + 1:] == off, "exactly one extra call, everything else as it was"
    lm_head = max(i for i, name in enumerate(got) if name.startswith("umv_gemm"))
    assert at > lm_head
    if "umv_logit_penalty_bf16" in got:
        assert at == got.index("umv_logit_penalty_bf16") + 1
    else:
        assert at == lm_head + 1
    if "umv_logit_constrain_bf16" in got:
        assert at == got.index("umv_logit_constrain_bf16") - 1
    # the structure the call was given
    a = args[0][0]._obj
    assert (a.M, a.V, a.hist_ld) == (2, D.VOCAB, s_on.ng_hist.shape[1]) and a.hist == s_on.ng_hist.data_ptr() and a.hist_len == s_on.ng_len.data_ptr()
    assert a.ids == s_on.ids.data_ptr() and a.logits == s_on.logits.data_ptr()
    if rows:
        assert a.n == 0 and a.row_n == s_on.ng_row_n.data_ptr() and s_on.ng_row_n.tolist() == [3, 1] and a.rows == s_on.row_table.data_ptr()
    else:
        assert a.n == 3 and not a.row_n and s_on.ng_len.tolist() == [3, 1] and s_on.ng_hist[0, :3].tolist() == [4, 5, 4]
    assert bool(a.argmax_partial) == s_on.fused_argmax
    assert any(t is s_on.ng_hist for t in s_on._state()) and any(t is s_on.ng_len for t in s_on._state())
