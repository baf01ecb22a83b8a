"""Constrained decoding (include/unimedvl_hip.h, "token automata"), the parts that need no GPU: the builders of
unimedvl_amd.constraints, `walk` as the host model of the advance kernel, validation, the tests' numpy model (tests/constraint_ref.py)
against a brute-force restatement, the public keywords, and the ABI."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import constraint_ref as C
import penalty_ref as P
from unimedvl_amd.constraints import FREE, LEFT, TokenAutomaton

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = 3


def _edges(a, s):
    return dict(zip(a.edge_token[a.row_ptr[s]:a.row_ptr[s + 1]].tolist(), a.edge_next[a.row_ptr[s]:a.row_ptr[s + 1]].tolist()))


# ----------------------------------------------------------------------------- builders
def test_choices_share_prefixes_and_are_sorted():
    a = TokenAutomaton.from_choices([[9, 1, 2], [5, 7], [5, 6]], EOS)
    # root: 5 and 9; the two choices that start with 5 share that state
    assert sorted(_edges(a, 0)) == [5, 9]
    five = _edges(a, 0)[5]
    assert sorted(_edges(a, five)) == [6, 7]
    # states: root, 9, 91, 912, 5, 57, 56 and the final one
    assert a.n_states == 8
    for s in range(a.n_states):
        t = a.edge_token[a.row_ptr[s]:a.row_ptr[s + 1]]
        assert t.size and (np.diff(t) > 0).all(), s
    assert a.row_ptr.dtype == a.edge_token.dtype == a.edge_next.dtype == np.int32
    final = a.n_states - 1
    assert _edges(a, final) == {EOS: final}                                   # the EOS self-loop
    for seq in ([9, 1, 2], [5, 7], [5, 6]):
        end = a.walk(0, seq)
        assert _edges(a, end) == {EOS: final}                                 # after a choice only EOS
        assert a.walk(0, seq + [EOS, EOS, EOS]) == final
    assert a.allowed(0).tolist() == [5, 9] and a.allowed(FREE) is None and a.allowed(a.n_states) is None


def test_a_choice_that_is_a_prefix_of_another():
    a = TokenAutomaton.from_choices([[5], [5, 6]], EOS)
    mid = a.walk(0, [5])
    assert sorted(_edges(a, mid)) == [EOS, 6]                                 # stop here, or go on
    final = a.n_states - 1
    assert a.walk(0, [5, EOS]) == final and a.walk(0, [5, 6, EOS]) == final and a.walk(0, [5, 6, 6]) == LEFT
    with pytest.raises(ValueError, match="prefix"):
        TokenAutomaton.from_choices([[5], [5, 6]], None, after="free")


def test_after_modes():
    stop = TokenAutomaton.from_choices([[5, 6], [8]], EOS, after="stop")
    free = TokenAutomaton.from_choices([[5, 6], [8]], None, after="free")
    assert stop.walk(0, [8]) >= 0 and stop.walk(0, [8, EOS]) == stop.n_states - 1
    assert free.walk(0, [8]) == FREE and free.walk(0, [5, 6]) == FREE and free.walk(0, [5]) >= 0
    assert free.walk(0, [5, 6, 77, 78]) == FREE                               # released: any text follows
    assert free.n_states == 2 and FREE in free.edge_next.tolist()
    for bad in ([[]], [[5], [5]], [], [[5, -1]], [[5, True]], [[5, 2.5]]):
        with pytest.raises(ValueError):
            TokenAutomaton.from_choices(bad, EOS)
    with pytest.raises(ValueError, match="eos_id"):
        TokenAutomaton.from_choices([[5, EOS]], EOS)
    with pytest.raises(ValueError, match="after"):
        TokenAutomaton.from_choices([[5]], EOS, after="maybe")
    with pytest.raises(ValueError):
        TokenAutomaton.from_choices([[5]], None, after="stop")


def test_allowed_tokens_and_union_offsets():
    one = TokenAutomaton.from_allowed_tokens([7, 3, 7, 11])
    assert one.n_states == 1 and one.allowed(0).tolist() == [3, 7, 11] and one.edge_next.tolist() == [0, 0, 0]
    assert one.walk(0, [3, 11, 7, 7]) == 0 and one.walk(0, [3, 4]) == LEFT
    with pytest.raises(ValueError):
        TokenAutomaton.from_allowed_tokens([])
    a = TokenAutomaton.from_choices([[5, 6], [8]], EOS)
    f = TokenAutomaton.from_choices([[5, 6], [8]], None, after="free")
    u, start = TokenAutomaton.union({"a": a, "one": one, "f": f})
    assert start == {"a": 0, "one": a.n_states, "f": a.n_states + 1} and u.n_states == a.n_states + 1 + f.n_states
    assert u.n_edges == a.n_edges + one.n_edges + f.n_edges
    for name, m in (("a", a), ("one", one), ("f", f)):
        for seq in ([5, 6, EOS, EOS], [8], [3, 7, 11], [5, 9], [5, 6, 1]):
            want = m.walk(0, seq, trace=True)
            got = u.walk(start[name], seq, trace=True)
            assert got == [w + start[name] if w >= 0 else w for w in want], (name, seq)
    with pytest.raises(ValueError):
        TokenAutomaton.union({})


def test_walk_leaves_on_a_foreign_token_and_stays_out():
    a = TokenAutomaton.from_choices([[5, 6], [8]], EOS)
    assert a.walk(0, [5, 9, 6, EOS, 5], trace=True)[1:] == [LEFT] * 4
    assert a.walk(LEFT, [5, 6]) == LEFT and a.walk(FREE, [5, 6]) == FREE and a.walk(a.n_states + 3, [5]) == a.n_states + 3
    assert a.step(0, 5) == a.walk(0, [5])


def test_validation_errors():
    ok = ([0, 2, 3], [4, 9, 1], [1, 0, FREE])
    TokenAutomaton(*ok)
    for bad in (([0, 2, 3], [9, 4, 1], [1, 0, 0]),          # unsorted within a state
                ([0, 2, 3], [4, 4, 1], [1, 0, 0]),          # a repeated token
                ([0, 2, 3], [4, 9, 1], [1, 2, 0]),          # a next state that does not exist
                ([0, 2, 3], [4, 9, 1], [1, -2, 0]),         # below FREE
                ([0, 2, 3], [4, -9, 1], [1, 0, 0]),         # a negative token
                ([1, 2, 3], [4, 9, 1], [1, 0, 0]),          # row_ptr does not start at 0
                ([0, 2, 2], [4, 9, 1], [1, 0, 0]),          # ... or end at the edge count
                ([0, 3, 2, 3], [4, 9, 1], [1, 0, 0]),       # ... or descends
                ([0, 2, 3], [4, 9, 1], [1, 0]),             # lengths
                ([0], [], []),                              # no state
                ([0, 2, 2, 3], [4, 9, 1], [1, 0, 0])):      # a state without edges
        with pytest.raises(ValueError):
            TokenAutomaton(*bad)
    e = TokenAutomaton([0, 2, 2, 3], [4, 9, 1], [1, 0, 0], allow_empty_states=True)      # legal for the kernels
    assert e.allowed(1).size == 0 and e.walk(1, [4]) == LEFT


# ----------------------------------------------------------------------------- the model against a brute-force restatement
def _random_automaton(rng, n_states, V, over=0):
    """random edge sets, tokens up to V + over - 1 (those >= V must be ignored by the mask), some next states FREE"""
    states = []
    for s in range(n_states):
        k = int(rng.integers(1, 9))
        toks = rng.choice(V + over, size=k, replace=False).tolist()
        states.append([(int(t), int(rng.integers(-1, n_states))) for t in toks])
    return C.Automaton.from_states(states)


@pytest.mark.parametrize("V", [40, 330])
def test_model_against_brute_force(V):
    rng = np.random.default_rng(V)
    for trial in range(20):
        ref = _random_automaton(rng, 6, V, over=7)
        host = TokenAutomaton(*ref.arrays())
        bits = P.bf16_bits((rng.standard_normal(V) * 3).astype(np.float32))
        bits[rng.integers(0, V, 3)] = 0xFF80                                  # -inf
        bits[rng.integers(0, V, 2)] = 0x7FC0                                  # NaN
        for s in (-2, -1, 0, 3, 5, 6, 99):
            got = C.mask_row(bits, ref, s)
            if ref.free(s):
                assert np.array_equal(got, bits) and host.allowed(s) is None
                continue
            A = [t for t, _ in ref.edges(s) if t < V]
            assert A == [t for t in host.allowed(s).tolist() if t < V] == ref.allowed(s, V)
            for n in range(V):                                                # the definition, column by column
                assert got[n] == (bits[n] if n in A else 0xFF80)
            if not A:
                continue
            for T in (0.0, 0.7):
                for tok in A:
                    a, b = C.logprob(got, tok, T), C.restricted_logprob(bits, A, tok, T)
                    assert (np.isnan(a) and np.isnan(b)) or a == b or abs(a - b) < 1e-12
            top = int(C.greedy_keys(got).max())
            assert 0xFFFFFFFF - (top & 0xFFFFFFFF) == C.restricted_argmax(bits, A)
            m, ssum = C.tile_stats(got)
            for t in range(len(m)):
                if not any(16 * t <= n < 16 * t + 16 for n in A):
                    assert m[t] == -np.inf and ssum[t] == 0
        toks = rng.integers(0, V + 7, 12).tolist()
        for s0 in (0, 2, -1):
            assert ref.walk(s0, toks) == host.walk(s0, toks, trace=True)
        # a walk that follows edges for a while, so that not every walk ends in LEFT at once
        s, path = 0, []
        for _ in range(6):
            if ref.free(s):
                break
            t, _ = ref.edges(s)[int(rng.integers(0, len(ref.edges(s))))]
            path.append(t)
            s = ref.step(s, t)
        assert ref.walk(0, path) == host.walk(0, path, trace=True) and (not path or ref.walk(0, path)[-1] == s)


# ----------------------------------------------------------------------------- public surface
def test_keywords_exist_default_off_and_sit_before_top_k():
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.decode import DecodeSession
    from unimedvl_amd.interactive_vqa_inferencer import DEFAULT_CONFIG, VQAInferencer
    from unimedvl_amd.serving import ContinuousBatcher
    for fn, names in ((DecodeSession.__init__, ("constraint", "constraint_states")), (Bagel.generate_text, ("constraint", "constraint_states")),
                      (Bagel.chat, ("choices",)), (ContinuousBatcher.__init__, ("constraints",)), (VQAInferencer.infer_single, ("choices",))):
        p = inspect.signature(fn).parameters
        order = list(p)
        for n in names:
            assert p[n].default is None and p[n].kind is inspect.Parameter.KEYWORD_ONLY, (fn.__qualname__, n)
            assert order.index(n) < order.index("top_k"), (fn.__qualname__, n)
        assert order[-3:] == ["top_k", "top_p", "min_p"], fn.__qualname__
    assert inspect.signature(Bagel.chat).parameters["choices_after"].default == "stop"
    assert DEFAULT_CONFIG["choices"] is None and DEFAULT_CONFIG["choices_after"] == "stop"
    assert inspect.signature(ContinuousBatcher.submit).parameters["constraint"].default is None
    assert inspect.signature(DecodeSession.set_slot).parameters["constraint_state"].default is None
    with pytest.raises(ValueError, match="constraint"):                       # before anything touches a device
        DecodeSession(None, None, None, None, 4, constraint_states=[0])


def test_speculative_session_refuses_a_constraint():
    from unimedvl_amd.speculative import SpeculativeDecodeSession

    class Cache:
        lens = [4]
    a = TokenAutomaton.from_allowed_tokens([1, 2])
    with pytest.raises(ValueError, match="constraint"):
        SpeculativeDecodeSession(None, Cache(), None, None, 8, 2, constraint=a)


def test_binding_header_and_driver_carry_both_entries():
    from unimedvl_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "unimedvl_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    drv = open(os.path.join(ROOT, "tools", "abi_sanitize_driver.cpp")).read()
    for name in ("umv_logit_constrain_bf16", "umv_constraint_advance"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in _lib._SIGS, name
        assert re.search(r"EXPECT_ERR\(" + name + r"\(nullptr", drv), name     # NULL arguments
        assert re.search(r"EXPECT_OK\(" + name + r"\(", drv), name             # a valid call
        assert len(re.findall(name + r"\(", drv)) >= 5, name                    # and invalid ones
    assert len(_lib._SIGS["umv_constraint_advance"][1]) == 5
    assert int(re.search(r"#define UMV_CONSTRAIN_CHUNK (\d+)", src).group(1)) == ops.CONSTRAIN_CHUNK == _lib.CONSTRAIN_CHUNK
    assert ops.CONSTRAIN_CHUNK % 16 == 0
    assert (int(re.search(r"#define UMV_CONSTRAINT_FREE \((-\d+)\)", src).group(1)), int(re.search(r"#define UMV_CONSTRAINT_LEFT \((-\d+)\)", src).group(1))) \
        == (FREE, LEFT) == (_lib.CONSTRAINT_FREE, _lib.CONSTRAINT_LEFT) == (C.FREE, C.LEFT)
    assert "logit_constrain.hip" in __import__("unimedvl_amd.build", fromlist=["SOURCES"]).SOURCES[-1]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_ctypes_structs_match_the_header(tmp_path):
    from unimedvl_amd import _lib
    fields = {"umv_token_automaton": _lib.TokenAutomatonArgs, "umv_logit_constrain_args": _lib.LogitConstrainArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "unimedvl_hip.h"', "int main(void) {"]
    for cs, cls in fields.items():
        lines.append(f'  printf("{cs} size %zu\\n", sizeof({cs}));')
        for f, _ in cls._fields_:
            lines.append(f'  printf("{cs} {f} %zu\\n", offsetof({cs}, {f}));')
    lines += ["  return 0;", "}"]
    (tmp_path / "abi.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "abi"), str(tmp_path / "abi.c")])
    c = {}
    for ln in subprocess.check_output([str(tmp_path / "abi")], text=True).splitlines():
        s, f, v = ln.split()
        c.setdefault(s, {})[f] = int(v)
    for cs, cls in fields.items():
        assert ctypes.sizeof(cls) == c[cs]["size"], cs
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == c[cs][f], (cs, f)
