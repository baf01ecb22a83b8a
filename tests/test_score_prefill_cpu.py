"""The prefill-time scorer (Bagel.score_prefill; include/unimedvl_hip.h, "token log-probabilities of given rows"), the parts that need no
GPU: the two entry points in header and binding with matching signatures, the row / target layout and the lm_head chunk plan against
plain-Python statements, the host-side refusals, and the public parameter lists."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("umv_lm_head_stats_bf16", "umv_token_logprob_from_stats")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "unimedvl_hip.h")).read(), flags=re.S)


def _ctype_of(decl):
    """one C parameter declaration -> the ctypes type the binding must give it"""
    from unimedvl_amd import _lib
    decl = decl.strip()
    if re.match(r"const\s+umv_gemm_args\s*\*", decl):
        return ctypes.POINTER(_lib.GemmArgs)
    if "*" in decl or re.match(r"umv_stream_t\b", decl):
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[decl.split()[0]]


def test_header_and_binding_signatures():
    from unimedvl_amd import _lib, build
    hdr = _header()
    for name in ENTRIES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in the header"
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int
        assert args == [_ctype_of(d) for d in m.group(1).split(",")], name
    # the header's parameter names, in order: the struct first and unchanged, the pointers behind it
    names = lambda n: [d.split()[-1].lstrip("*") for d in re.search(n + r"\s*\(([^)]*)\)", hdr).group(1).split(",")]   # noqa: E731
    assert names("umv_lm_head_stats_bf16") == ["a", "ids", "lse_partial", "target_y", "stream"]
    assert names("umv_token_logprob_from_stats") == ["lse_partial", "n_tiles", "target_y", "ids", "V", "out", "M", "stream"]
    assert [n for n, _ in _lib.GemmArgs._fields_][-1] == "lse_partial"          # umv_gemm_args keeps its layout: nothing appended
    assert "lm_head_stats.hip" in build.SOURCES + build.LAST_SOURCES + build.TAIL_SOURCES
    drv = open(os.path.join(ROOT, "tools", "abi_sanitize_driver.cpp")).read()
    for name in ENTRIES:
        assert re.search(r"EXPECT_ERR\(" + name + r"\(nullptr", drv) and len(re.findall(name + r"\(", drv)) >= 3, name


# ----------------------------------------------------------------------------- the row and target layout
def _layout_by_hand(cands, append_eos, eos, start, pos0):
    """candidate tokens t_0 .. t_{m-1} behind a context: row i is fed [start, t_0, ..][i] at rope position pos0 + i and scored against t_i"""
    rows = []
    for c in cands:
        t = list(c) + ([eos] if append_eos else [])
        for i in range(len(t)):
            rows.append((start if i == 0 else t[i - 1], t[i], pos0 + i))
    return rows


@pytest.mark.parametrize("append_eos", [True, False])
def test_row_and_target_layout(append_eos):
    from unimedvl_amd.bagel import Bagel, prefill_score_layout
    eos, start, pos0 = 301, 300, 37
    cands = [[7], [5, 6, 7, 8, 9, 10, 11], [9, 9], list(range(20, 60))]                     # ragged: 1, 7, 2 and 40 tokens
    toks = Bagel._score_candidates(None, {"eos_token_id": eos}, cands, append_eos)
    assert toks == [list(c) + ([eos] if append_eos else []) for c in cands]
    fed, targets, qlens, pos = prefill_score_layout(toks, start, pos0)
    assert qlens == [len(t) for t in toks] and len(fed) == len(targets) == len(pos) == sum(qlens)
    assert list(zip(fed, targets, pos)) == _layout_by_hand(cands, append_eos, eos, start, pos0)
    # every candidate starts on the start token at the context's position, and its last token is a target only
    r0 = 0
    for t in toks:
        assert fed[r0] == start and pos[r0] == pos0 and targets[r0 + len(t) - 1] == t[-1] and pos[r0 + len(t) - 1] == pos0 + len(t) - 1
        r0 += len(t)


class _Tok:
    def encode(self, s):
        return [int(v) for v in s.split()]


def test_candidate_handling_is_scores():
    from unimedvl_amd.bagel import Bagel
    ids = {"eos_token_id": 301}
    assert Bagel._score_candidates(_Tok(), ids, ["7 8", [9]], True) == [[7, 8, 301], [9, 301]]
    assert Bagel._score_candidates(_Tok(), ids, ["7 8", (9,)], False) == [[7, 8], [9]]
    with pytest.raises(ValueError, match="64"):
        Bagel._score_candidates(_Tok(), ids, [[7]] * 65, True)
    with pytest.raises(ValueError, match="64"):
        Bagel._score_candidates(_Tok(), ids, [], True)
    with pytest.raises(ValueError, match="empty"):
        Bagel._score_candidates(_Tok(), ids, [[7], []], False)
    assert len(Bagel._score_candidates(_Tok(), ids, [[7]] * 64, True)) == 64


# ----------------------------------------------------------------------------- the chunk plan
@pytest.mark.parametrize("rows_per_pass", [1, 7, 1024])
@pytest.mark.parametrize("T", [0, 1, 6, 7, 8, 50, 1024, 1025, 2300])
def test_chunk_plan(T, rows_per_pass):
    from unimedvl_amd.llm import row_chunks
    plan = row_chunks(T, rows_per_pass)
    assert [r for r0, r1 in plan for r in range(r0, r1)] == list(range(T))                 # every row once, in order
    assert all(0 < r1 - r0 <= rows_per_pass for r0, r1 in plan)
    assert len(plan) == (T + rows_per_pass - 1) // rows_per_pass                           # no pass more than needed
    assert all(r1 - r0 == rows_per_pass for r0, r1 in plan[:-1])                           # only the last pass is short


def test_workspace_bytes():
    from unimedvl_amd.llm import token_logprobs_workspace_bytes
    V = 152064
    assert token_logprobs_workspace_bytes(1, V, True) == 9504 * 8 + 4                      # 76 KB of statistics and one logit per row
    assert token_logprobs_workspace_bytes(1, V, False) == 2 * V                            # 304 KB of logits per row
    assert token_logprobs_workspace_bytes(1024, V, True) < 80e6 < 300e6 < token_logprobs_workspace_bytes(1024, V, False)


# ----------------------------------------------------------------------------- refusals on the host
def test_refusals():
    from unimedvl_amd import ops
    from unimedvl_amd.llm import fused_lm_head_ok, row_chunks
    for bad in (0, -1, 2.5, True, "8"):
        with pytest.raises((ValueError, TypeError)):
            row_chunks(10, bad)
    lin = ops.PackedLinear(torch.zeros(1), None, 1000, 512)
    assert fused_lm_head_ok(lin)
    for kw in (dict(w8=torch.zeros(1), scale=torch.zeros(1)), dict(w4=torch.zeros(1)), dict(th=12), dict(swiglu=True)):
        assert not fused_lm_head_ok(ops.PackedLinear(torch.zeros(1), None, 1000, 512, **kw)), kw
    assert not fused_lm_head_ok(ops.PackedLinear(None, None, 1000, 512, w4=torch.zeros(1)))


# ----------------------------------------------------------------------------- the public interface
def test_public_parameter_lists():
    from unimedvl_amd import ops
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.interactive_vqa_inferencer import VQAInferencer
    from unimedvl_amd.llm import Qwen2MoT
    sc = inspect.signature(Bagel.score).parameters                                         # `score` is pinned
    assert list(sc)[1:] == ["tokenizer", "new_token_ids", "image_transform", "images", "prompt", "candidates", "append_eos"]
    assert sc["append_eos"].default is True
    assert list(inspect.signature(Bagel.score_top_logprobs).parameters)[1:] == list(sc)[1:] + ["top_logprobs"]
    sp = inspect.signature(Bagel.score_prefill).parameters
    assert list(sp)[1:] == list(sc)[1:] + ["rows_per_pass", "fused"]                       # score's list, then the new keywords
    assert sp["append_eos"].default is True and sp["rows_per_pass"].default == 1024 and sp["fused"].default is True
    assert all(sp[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("rows_per_pass", "fused"))
    assert all(sp[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for k in list(sc)[1:])
    assert list(inspect.signature(VQAInferencer.score).parameters)[1:] == ["image", "question", "candidates", "append_eos"]
    assert list(inspect.signature(VQAInferencer.score_prefill).parameters)[1:] == ["image", "question", "candidates", "append_eos"]
    tl = inspect.signature(Qwen2MoT.token_logprobs).parameters
    assert list(tl)[1:] == ["hidden", "target_ids", "rows_per_pass", "fused"] and tl["rows_per_pass"].default == 1024
    assert tl["fused"].kind is inspect.Parameter.KEYWORD_ONLY and tl["fused"].default is True
    assert "score_prefill" in Bagel.score.__doc__                                           # the forced scorer points to the new method
    assert callable(ops.lm_head_stats) and callable(ops.token_logprob_from_stats)
