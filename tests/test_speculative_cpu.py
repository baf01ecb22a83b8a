"""Speculative greedy decode without a GPU: the plain-Python model of the step end (tests/spec_ref.py) on hand-written lookup cases and
driven by a toy deterministic model - whatever the drafts, the emitted sequence is the plain greedy one - plus the C ABI of
umv_decode_step_end_speculative (header, ctypes mirror, _SIGS, the sanitizer driver) and the keywords on the public interface."""
import ctypes
import inspect
import os
import random
import re
import shutil
import subprocess

import pytest

import spec_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unimedvl_hip.h")
V = 50


# ----------------------------------------------------------------------------- prompt lookup, by hand
def test_longest_ngram_wins_over_a_later_shorter_match():
    #        0  1  2  3  4  5  6  7  8  9 10 11
    hist = [1, 2, 3, 4, 9, 9, 3, 4, 7, 2, 3, 4]
    # suffix (2, 3, 4) occurs at 1 -> continuation 9 9 3; the shorter suffix (3, 4) occurs later, at 6 -> 7 2 3
    assert S.lookup(hist, 3, 2, 3, V) == [9, 9, 3]
    assert S.lookup(hist, 3, 2, 2, V) == [7, 2, 3]
    assert S.lookup(hist, 3, 1, 1, V) == [7, 2, 3]          # (4) alone: most recent earlier 4 is at 7


def test_most_recent_match_wins():
    hist = [5, 6, 1, 5, 6, 2, 5, 6, 3, 5, 6]
    assert S.lookup(hist, 2, 2, 4, V) == [3, 5]
    assert S.lookup(hist[:8], 2, 2, 4, V) == [2, 5]


def test_continuation_runs_into_the_tail():
    hist = [7, 8, 9, 7, 8]
    assert S.lookup(hist, 7, 2, 4, V) == [9, 7, 8]          # three tokens exist behind the match, not seven
    hist = [7, 8, 7, 8]
    assert S.lookup(hist, 3, 2, 2, V) == [7, 8]
    assert S.lookup([4, 4, 4], 5, 2, 2, V) == [4]           # overlapping match at 0: one token behind it


def test_negative_separators():
    hist = [3, 4, -1, 3, 4]
    assert S.lookup(hist, 3, 2, 4, V) == []                 # the match at 0 decides, its continuation is a separator: no drafts
    assert S.lookup([3, -1, 5, 3, -1], 2, 2, 2, V) == []    # a suffix that holds a separator never matches
    assert S.lookup([3, -1, 5, 3, -1], 2, 1, 2, V) == []
    assert S.lookup([3, 4, 5, -1, 9, 3, 4], 3, 2, 2, V) == [5]     # drafts stop at the separator
    assert S.lookup([3, 4, 60, 6, 3, 4], 3, 2, 2, V) == []         # ... and at a token outside the vocabulary


def test_no_match_and_short_history():
    assert S.lookup([1, 2, 3, 4, 5], 3, 2, 4, V) == []
    assert S.lookup([1], 3, 1, 4, V) == []                  # history no longer than ngram_min
    assert S.lookup([1, 1], 3, 2, 4, V) == []
    assert S.lookup([], 3, 1, 2, V) == []
    assert S.lookup([1, 1], 3, 1, 4, V) == [1]


def test_predicted_continuation():
    pred = [5, 6, 7, 8]
    assert S.from_predicted(pred, 4, 0, 3, V) == [5, 6, 7]
    assert S.from_predicted(pred, 4, 2, 3, V) == [7, 8]     # shorter than the window
    assert S.from_predicted(pred, 3, 2, 3, V) == [7]
    assert S.from_predicted(pred, 4, 4, 3, V) == []
    assert S.from_predicted([5, V, 7], 3, 0, 3, V) == [5]   # a token outside the vocabulary ends the drafts
    assert S.from_predicted([5, -1, 7], 3, 0, 3, V) == [5]


# ----------------------------------------------------------------------------- the loop, with a toy model
def _toy(seed):
    """a deterministic next-token function with some repetition in it: mostly a hash of the last two tokens, over a small alphabet"""
    def nxt(seq):
        a, b = seq[-1], seq[-2] if len(seq) > 1 else 0
        return (a * 7 + b * 3 + seed + (len(seq) // 11)) % 6 + 1
    return nxt


CONTEXT = [1, 2, 3, 1, 2, 4, -1, 5, 1, 2]


def _sample(k, limit, out_ld=40, predicted=None, ngram=(2, 4), hist_ld=128):
    s = S.Sample(k, 3, slot=10, pos=17, out_ld=out_ld, limit=limit, hist=CONTEXT + [3], hist_ld=hist_ld, vocab=V, ngram=ngram,
                 predicted=predicted, pred_len=0 if predicted is None else len(predicted))
    s.draft()
    return s


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("drafts", ["lookup", "perfect", "random", "adversarial", "off_by_one", "empty"])
def test_any_drafts_give_the_plain_greedy_sequence(k, drafts):
    rng = random.Random(k * 100 + len(drafts))
    for seed in range(5):
        nxt = _toy(seed)
        for limit in (1, 2, k, k + 1, k + 2, 23, 24):
            plain = S.plain_greedy(nxt, CONTEXT, 3, limit)
            predicted = redraft = None
            if drafts == "perfect":
                predicted = plain
            elif drafts == "off_by_one":          # right except every third token
                predicted = [t if i % 3 != 1 else t % 6 + 1 for i, t in enumerate(plain)]
            elif drafts == "empty":
                predicted = [-1] * limit
            elif drafts in ("random", "adversarial"):
                def redraft(s, adversarial=drafts == "adversarial"):
                    true = S.plain_greedy(nxt, CONTEXT, 3, s.n_out + s.k + 1)[s.n_out:]
                    n = rng.randint(0, s.k)
                    d = [rng.randint(1, 6) for _ in range(n)]
                    if adversarial and n:           # right up to one position, then wrong, then right again
                        bad = rng.randrange(n)
                        d = [true[j] if j != bad else true[j] % 6 + 1 for j in range(n)]
                    s.ids = [s.ids[0]] + d + [s.ids[0]] * (s.k - n)
                    s.n_draft = n
            s = _sample(k, limit, predicted=predicted)
            steps = S.run(s, nxt, CONTEXT, redraft=redraft)
            assert s.out[:s.n_out] == plain and s.n_out == limit, (drafts, seed, limit)
            assert s.kv_len == 10 + limit + k + 1 and s.tok_slot == [10 + limit + j for j in range(k + 1)]
            assert s.tok_pos == [17 + limit + j for j in range(k + 1)]
            assert s.hist[:s.hist_len] == CONTEXT + [3] + plain
            assert s.stats[0] == steps and s.stats[2] <= s.stats[1] <= steps * k
            if drafts == "perfect":
                assert steps == S.steps_for(limit, k) and s.stats[1] == s.stats[2]
            if drafts == "empty":
                assert steps == limit and s.stats[1] == 0


@pytest.mark.parametrize("k", [1, 3, 7])
def test_limit_edge_and_m_zero(k):
    nxt = _toy(2)
    plain = S.plain_greedy(nxt, CONTEXT, 3, 30)
    s = _sample(k, limit=5, predicted=plain)
    S.run(s, nxt, CONTEXT)
    assert s.n_out == 5 and s.out[:5] == plain[:5]
    before = (list(s.out), s.n_out, s.kv_len, list(s.tok_slot), list(s.tok_pos), s.ids[0], s.hist_len)
    picks = [nxt(CONTEXT + [3] + plain[:5] + s.ids[1:j + 1]) for j in range(k + 1)]
    n, m = s.step_end(picks)             # at the limit: nothing is emitted, nothing moves, the step is counted
    assert m == 0 and (list(s.out), s.n_out, s.kv_len, list(s.tok_slot), list(s.tok_pos), s.ids[0], s.hist_len) == before
    s.limit = 9                           # the host raises the limit between replays: decoding goes on where it stopped
    S.run(s, nxt, CONTEXT)
    assert s.out[:9] == plain[:9]
    # out_ld clips like the limit does
    s = _sample(k, limit=100, out_ld=6, predicted=plain)
    S.run(s, nxt, CONTEXT)
    assert s.n_out == 6 and s.out == plain[:6]
    # a history that is full drops tokens and still decodes the same sequence
    s = _sample(k, limit=12, hist_ld=len(CONTEXT) + 3)
    S.run(s, nxt, CONTEXT)
    assert s.out[:12] == plain[:12] and s.hist_len == len(CONTEXT) + 3


# ----------------------------------------------------------------------------- the C ABI
def test_the_entry_point_is_bound_and_documented():
    from unimedvl_amd import _lib
    res, args = _lib._SIGS["umv_decode_step_end_speculative"]
    assert res is ctypes.c_int and len(args) == 2 and args[0]._type_ is _lib.SpecStepArgs
    text = open(HEADER).read()
    sec = text[text.index("speculative greedy decode"):text.index("int umv_decode_step_end_speculative")]
    for word in ("pick", "accept", "emit", "advance", "history", "draft", "predicted continuation", "prompt lookup", "FILLERS",
                 "draft_only", "UMV_ERR_ARG", "ngram_min", "rollback"):
        assert word in sec, word
    drv = open(os.path.join(ROOT, "tools", "abi_sanitize_driver.cpp")).read()
    assert "umv_decode_step_end_speculative(" in drv


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_ctypes_mirror_has_the_layout_of_the_header(tmp_path):
    from unimedvl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct\s*\{([^{}]*)\}\s*umv_spec_step_args\s*;", src).group(1)
    fields = [re.findall(r"[A-Za-z_][A-Za-z_0-9]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert fields == [n for n, _ in _lib.SpecStepArgs._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(umv_spec_step_args));']
    lines += [f'  printf("{f} %zu\\n", offsetof(umv_spec_step_args, {f}));' for f in fields] + ["  return 0;", "}"]
    (tmp_path / "abi.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-o", str(tmp_path / "abi"), str(tmp_path / "abi.c")])
    c = dict(ln.split() for ln in subprocess.check_output([str(tmp_path / "abi")], text=True).splitlines())
    assert ctypes.sizeof(_lib.SpecStepArgs) == int(c["size"])
    for f in fields:
        assert getattr(_lib.SpecStepArgs, f).offset == int(c[f]), f


def test_the_public_interface_carries_the_keywords():
    from unimedvl_amd import bagel, inferencer, speculative
    for fn in (bagel.Bagel.generate_text, bagel.Bagel.chat):
        p = inspect.signature(fn).parameters
        assert (p["draft_len"].default, p["draft_ngram"].default, p["predicted_ids"].default) == (0, (2, 4), None), fn
    assert inspect.signature(bagel.Bagel.generate_text).parameters["draft_context_ids"].default is None
    for fn in (inferencer.InterleaveInferencer.gen_text, inferencer.InterleaveInferencer.gen_text_batch):
        p = inspect.signature(fn).parameters
        assert (p["draft_len"].default, p["draft_ngram"].default, p["predicted_ids"].default) == (0, (2, 4), None), fn
    from unimedvl_amd.decode import DecodeSession
    assert issubclass(speculative.SpeculativeDecodeSession, DecodeSession)
