"""The C calls of a whole decode step (decode.DecodeSession / speculative.SpeculativeDecodeSession), what the session decided and
allocated, its host-written state and its refusals, pinned case by case against a table recorded from the PARENT of the commit that
folded the session's host layer - never from the tree under test.

A session runs on CPU tensors behind the seams of abi_recorder (use_graph=False, a two-layer stand-in model, a cache on "cpu"); no
kernel runs, so everything recorded is a pure function of the host code.  A recorded call is normalised: structures expanded field by
field, every pointer the name of what it points to - a session attribute, w.und[l].<name>.<image>, w.<name>, cache.slabs[l].k|vt|table,
constraint.<table> - plus a byte offset for a view, scalars literal.  A pointer that resolves to nothing is "?" and fails the test.  The
golden holds every distinct string once and each case as indices into that list.

    python tests/test_decode_step_calls_cpu.py --record      with PYTHONPATH = a checkout of the parent commit (git worktree add DIR <parent>):
                                                             rewrites tests/golden/decode_step_calls.json; refuses to record from this tree
    python tests/test_decode_step_calls_cpu.py --host-cost   microseconds per un-captured _step() under the recorder
                                                             (profiles/decode_plan_refactor.txt)
"""
import bisect
import contextlib
import ctypes as C
import functools
import json
import os
import sys
import timeit
from types import SimpleNamespace

import torch

from abi_recorder import _seams, render

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "decode_step_calls.json")
BF16 = torch.bfloat16
LAYERS, HIDDEN, HEADS, KV_HEADS, HEAD_DIM, INTER, VOCAB = 2, 64, 2, 1, 32, 128, 200      # vocab 200: 13 tiles, the last one partial
MAX_LENGTH = 4
ROW_COUNTS = (1, 2, 9, 33, 64, 65, 128, 129)    # both sides of nsplit's 8 / 32, of the fused step end's 64 and of split-K's 64 / 128
ENVS = ({"UMV_DECODE_FUSED_ARGMAX": "0"}, {"UMV_DECODE_SPLITK": "0"}, {"UMV_DECODE_SPLITK": "1,4,1"}, {"UMV_DECODE_EXACT_TILES": "0"},
        {"UMV_DECODE_NSPLIT": "1"}, {"UMV_DECODE_WSPLIT": "2"})
IMAGES = ("wp", "w8", "scale", "w8m", "w4", "wz", "bias")


def _model(ops, fp8=False):
    def E(*shape, dtype=BF16):
        return torch.empty(shape, dtype=dtype)

    def lin(N, K, bias=False, swiglu=False):
        return ops.PackedLinear(E(N * K), E(N) if bias else None, N, K, swiglu=swiglu)
    qkv = (HEADS + 2 * KV_HEADS) * HEAD_DIM
    und = [SimpleNamespace(qkv=lin(qkv, HIDDEN, bias=True), o=lin(HIDDEN, HEADS * HEAD_DIM), gate_up=lin(2 * INTER, HIDDEN, swiglu=True),
                           down=lin(HIDDEN, INTER), in_norm=E(HIDDEN), post_norm=E(HIDDEN), q_norm=E(HEAD_DIM), k_norm=E(HEAD_DIM))
           for _ in range(LAYERS)]
    w = SimpleNamespace(und=und, embed=E(VOCAB, HIDDEN), norm=E(HIDDEN), lm_head=lin(VOCAB, HIDDEN),
                        cos=E(4096, HEAD_DIM, dtype=torch.float32), sin=E(4096, HEAD_DIM, dtype=torch.float32))
    if fp8:
        w.fp8 = True
    cfg = SimpleNamespace(layers=LAYERS, hidden=HIDDEN, heads=HEADS, kv_heads=KV_HEADS, head_dim=HEAD_DIM, inter=INTER, vocab=VOCAB,
                          rms_eps=1e-6, max_position=4096)
    return SimpleNamespace(cfg=cfg, device="cpu", w=w)


def _cache(B, kv, paged=False):
    from unimedvl_amd.kvcache import NaiveCache, PagedCache
    if paged:
        cache = PagedCache(LAYERS, pool_pages=8, max_context=1024)
        cache.ensure_tokens([kv] * B, KV_HEADS, HEAD_DIM, "cpu")
    else:
        cache = NaiveCache(LAYERS)
        cache.ensure(B, kv, KV_HEADS, HEAD_DIM, "cpu")
    cache.lens = [kv] * B
    return cache


@functools.lru_cache(maxsize=None)
def _automaton():
    from unimedvl_amd.constraints import TokenAutomaton
    return TokenAutomaton.from_choices([[3, 4], [3, 7, 9], [11]], 199)


def _params(**kw):
    from unimedvl_amd.sampling import SamplingParams
    return SamplingParams(**kw)


def _mixed_rows():
    return [_params(), _params(do_sample=True, temperature=0.7, top_p=0.9, repetition_penalty=1.2, seed=11)]


def _forced():
    f = torch.full((MAX_LENGTH, 2), -1, dtype=torch.int64)
    f[1, 0] = 17
    return f


PENALTIES = dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25, logit_bias={7: -2.0, 150: 1.5},
                 penalty_context_ids=[[4, 5, 4], [6]], penalty_context_room=4)

# name -> (session keywords as a callable, {B, kv, spec, paged, fp8, env})
ARMS = {
    "greedy": (dict, {}),
    "do_sample": (lambda: dict(do_sample=True, temperature=0.7, seed=1234), {}),
    "logprobs": (lambda: dict(logprobs=True), {}),
    "forced_ids": (lambda: dict(forced_ids=_forced()), {}),
    "top_p logprobs": (lambda: dict(do_sample=True, temperature=0.7, seed=5, logprobs=True, top_p=0.9), {}),
    "top_k": (lambda: dict(do_sample=True, temperature=0.7, seed=5, top_k=5), {}),
    "penalties": (lambda: dict(PENALTIES), {}),
    "sampled penalties": (lambda: dict(PENALTIES, do_sample=True, temperature=0.8, seed=77), {}),
    "rows": (lambda: dict(row_sampling=_mixed_rows(), row_streams=[3, 4], seed=9, logit_bias={7: -2.0},
                          penalty_context_ids=[[4, 5], [6]], penalty_context_room=4), {}),
    "rows reserved": (lambda: dict(row_sampling=[_params(), _params(do_sample=True, top_k=4)], row_penalties=True, seed=9,
                                   penalty_context_room=4), {}),
    "top_logprobs greedy": (lambda: dict(top_logprobs=3), {}),
    "top_logprobs truncated": (lambda: dict(do_sample=True, temperature=0.7, seed=5, min_p=0.05, top_logprobs=3), {}),
    "top_logprobs rows": (lambda: dict(row_sampling=_mixed_rows(), top_logprobs=3), {}),
    "constraint greedy": (lambda: dict(constraint=_automaton(), constraint_states=[0, -1]), {}),
    "constraint sampled penalties": (lambda: dict(PENALTIES, do_sample=True, temperature=0.8, seed=77, constraint=_automaton(),
                                                  constraint_states=[0, -1]), {}),
    "speculative context": (lambda: dict(draft_len=2, draft_context_ids=[[1, 2, 3, 1, 2], [5, -1, 5]]), dict(spec=True)),
    "speculative predicted": (lambda: dict(draft_len=2, predicted_ids=[[8, 9, 10], [4]]), dict(spec=True)),
    "speculative sampled": (lambda: dict(draft_len=2, sampling=[_params(do_sample=True, temperature=0.7, top_k=5, seed=11), _params()],
                                         sampling_streams=[5, 6], logprobs=True, seed=3, draft_context_ids=[[1, 2, 3], [4]]),
                            dict(spec=True)),
    "speculative long": (lambda: dict(draft_len=2), dict(spec=True, kv=200)),
    "paged": (dict, dict(paged=True)),
    "greedy long": (dict, dict(kv=200)),
    "greedy fp8 B=65": (dict, dict(B=65, fp8=True)),
}
for _B in ROW_COUNTS:
    ARMS[f"greedy B={_B}"] = (dict, dict(B=_B))
    ARMS[f"greedy long B={_B}"] = (dict, dict(B=_B, kv=200))
    ARMS[f"do_sample B={_B}"] = (ARMS["do_sample"][0], dict(B=_B))
for _knob in ENVS:
    _tag = " ".join(f"{k}={v}" for k, v in _knob.items())
    ARMS[f"greedy long {_tag}"] = (dict, dict(kv=200, env=_knob))
    ARMS[f"sampled penalties long {_tag}"] = (ARMS["sampled penalties"][0], dict(kv=200, env=_knob))
# the arms whose host-written state is recorded: what set_slot takes there
STATE_ARMS = {"penalties": {}, "sampled penalties": {}, "rows": dict(sampling=True), "rows reserved": dict(sampling=True),
              "constraint greedy": dict(constraint_state=1), "constraint sampled penalties": dict(constraint_state=1)}


@contextlib.contextmanager
def _env(env):
    keys = [k for k in os.environ if k.startswith("UMV_DECODE_")] + list(env)
    saved = {k: os.environ.get(k) for k in keys}
    for k in saved:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _session(ops, arm, **over):
    from unimedvl_amd.decode import DecodeSession
    from unimedvl_amd.speculative import SpeculativeDecodeSession
    make, opt = ARMS[arm]
    B, kv = opt.get("B", 2), opt.get("kv", 5)
    kw = dict(make(), **over)
    llm, cache = _model(ops, opt.get("fp8", False)), _cache(B, kv, opt.get("paged", False))
    start, pos = torch.arange(B, dtype=torch.int64) + 20, torch.full((B,), kv, dtype=torch.int64)
    if opt.get("spec"):
        return SpeculativeDecodeSession(llm, cache, start, pos, MAX_LENGTH, kw.pop("draft_len"), use_graph=False, **kw)
    return DecodeSession(llm, cache, start, pos, MAX_LENGTH, use_graph=False, **kw)


def _names(sess):
    """[(first byte, one past the last, name)] of everything a call may point into, sorted; the first name of an address wins"""
    named = []

    def add(name, v):
        if isinstance(v, torch.Tensor):
            named.append((name, v))
        elif hasattr(v, "wp") and hasattr(v, "N"):        # a PackedLinear
            for f in IMAGES:
                add(f"{name}.{f}", getattr(v, f))
    for name, v in vars(sess).items():
        add(name, v)
    w = sess.llm.w
    for l, lw in enumerate(w.und):
        for name, v in vars(lw).items():
            add(f"w.und[{l}].{name}", v)
    for l, copies in enumerate(getattr(w, "decode_copies", ())):
        for i, v in enumerate(copies):
            add(f"w.decode_copies[{l}][{i}]", v)
    for name, v in vars(w).items():
        add(f"w.{name}", v)
    for l, slab in enumerate(sess.cache.slabs):
        for f in ("k", "vt", "table"):
            add(f"cache.slabs[{l}].{f}", getattr(slab, f, None))
    if sess.con_dev is not None:
        for f in ("row_ptr", "edge_token", "edge_next"):
            add(f"constraint.{f}", getattr(sess.con_dev, f))
    spans, seen = [], set()
    for name, t in named:
        if t.numel() and t.data_ptr() not in seen:
            seen.add(t.data_ptr())
            spans.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), name))
    return sorted(spans)


def _render(calls, spans):
    starts = [s[0] for s in spans]

    def find(v):
        i = bisect.bisect_right(starts, v) - 1
        return spans[i] if i >= 0 and v < spans[i][1] else None

    def ptr(v):
        v = v.value if isinstance(v, C.c_void_p) else v
        if v is None:
            return "0"
        hit = find(v)
        return "?" if hit is None else hit[2] if v == hit[0] else f"{hit[2]}+{v - hit[0]}"
    return render(calls, ptr, lambda v: isinstance(v, int) and not isinstance(v, bool) and find(v) is not None)


def _plan(sess):
    return dict(step_end=sess.step_end, lm_head_kw=sorted(sess.lm_head_kw), sk=list(sess.sk), nsplit=sess.nsplit,
                fused_argmax=sess.fused_argmax,
                tensors={a: [str(v.dtype), list(v.shape)] for a, v in sorted(vars(sess).items()) if isinstance(v, torch.Tensor)})


def _case(ops, calls, arm):
    """{"ctor": [...], "step": [...], "step2": [...], "plan": {...}} of one arm"""
    del calls[:]
    with _env(ARMS[arm][1].get("env", {})):
        sess = _session(ops, arm)
        n0 = len(calls)
        sess.step(1)
        n1 = len(calls)
        sess.step(1)
    spans = _names(sess)
    return dict(ctor=_render(calls[:n0], spans), step=_render(calls[n0:n1], spans), step2=_render(calls[n1:], spans), plan=_plan(sess))


def _snapshot(sess):
    names = [a for t in sess._state() for a, v in vars(sess).items() if v is t] + ["pen_bias", "row_table"]
    return {a: getattr(sess, a).tolist() for a in dict.fromkeys(names) if getattr(sess, a, None) is not None}


def _states(ops, arm):
    """the host-written state of an arm after construction, set_slot, rewind_outputs and the copy_* methods"""
    takes = STATE_ARMS[arm]
    out = {}
    sess = _session(ops, arm)
    out["construction"] = _snapshot(sess)
    kw = dict(penalty_context_ids=[4, 5])
    if takes.get("sampling"):
        kw.update(sampling=_params(do_sample=True, temperature=0.5, top_k=3, seed=21), stream=7, draw=2)
    if "constraint_state" in takes:
        kw.update(constraint_state=takes["constraint_state"])
    sess.set_slot(1, 9, 3, 3, **kw)
    out["set_slot"] = _snapshot(sess)
    sess.rewind_outputs()
    out["rewind_outputs"] = dict(_snapshot(sess), in_ids=sess.in_ids.tolist(), steps_done=sess.steps_done)
    for slots in (None, [1]):
        over = {}
        if sess.pen is not None:
            over.update(penalty_context_room=2, penalty_context_ids=[[8], [9, 10]])
        if sess.con_state is not None:
            over.update(constraint_states=[2, 1])
        other, into = _session(ops, arm, **over), _session(ops, arm)
        into.copy_penalty_history(other, slots)
        into.copy_constraint_states(other, slots)
        out[f"copy slots={slots}"] = _snapshot(into)
    return out


def _refusals(ops):
    from unimedvl_amd.decode import DecodeSession
    S = functools.partial(_session, ops)
    cases = {
        "logprobs at B=65": lambda: S("greedy B=65", logprobs=True),
        "truncation without do_sample": lambda: S("greedy", top_k=5),
        "temperature 0 with truncation": lambda: S("greedy", do_sample=True, temperature=0.0, top_k=5),
        "row_streams without row_sampling": lambda: S("greedy", row_streams=[0, 1]),
        "row_penalties without row_sampling": lambda: S("greedy", row_penalties=True),
        "constraint_states without constraint": lambda: DecodeSession(None, None, None, None, 4, constraint_states=[0]),
        "bad forced_ids shape": lambda: S("greedy", forced_ids=torch.zeros((MAX_LENGTH, 3), dtype=torch.int64)),
        "forced_ids outside the vocabulary": lambda: S("greedy", forced_ids=torch.full((MAX_LENGTH, 2), VOCAB, dtype=torch.int64)),
        "set_slot context longer than the room": lambda: S("penalties").set_slot(1, 9, 3, 3, penalty_context_ids=[1, 2, 3, 4, 5]),
        "set_slot(sampling=) on a scalar session": lambda: S("greedy").set_slot(1, 9, 3, 3, sampling=_params()),
        "set_slot(constraint_state=) without constraint": lambda: S("greedy").set_slot(1, 9, 3, 3, constraint_state=0),
        "penalised row without penalty buffers": lambda: S("top_logprobs rows", row_sampling=[_params(), _params()]).set_slot(
            1, 9, 3, 3, sampling=_params(presence_penalty=0.5)),
        "row_sampling of the wrong length": lambda: S("greedy", row_sampling=[_params()]),
        "constraint_states of the wrong length": lambda: S("greedy", constraint=_automaton(), constraint_states=[0]),
        "penalty_context_ids of the wrong length": lambda: S("greedy", presence_penalty=0.5, penalty_context_ids=[[1]]),
        "speculative draft_len=0": lambda: S("speculative context", draft_len=0),
        "speculative B * (k + 1) > 64": lambda: S("speculative context", draft_len=40),
        "speculative set_slot": lambda: S("speculative context").set_slot(1, 9, 3, 3),
        "speculative rewind_outputs": lambda: S("speculative context").rewind_outputs(),
        "speculative sampling_streams without sampling": lambda: S("speculative context", sampling_streams=[0, 1]),
        "speculative sampling of the wrong length": lambda: S("speculative context", sampling=[_params()]),
        "speculative penalised sampling": lambda: S("speculative context", sampling=_params(presence_penalty=0.5)),
        "speculative unexpected keyword": lambda: S("speculative context", no_such_keyword=1),
    }
    for name, value in dict(do_sample=True, temperature=0.7, top_k=5, top_p=0.9, min_p=0.1, repetition_penalty=1.2, presence_penalty=0.5,
                            frequency_penalty=0.5).items():
        cases[f"row_sampling with {name}"] = functools.partial(S, "top_logprobs rows", **{name: value})
    off = dict(do_sample=True, logprobs=True, forced_ids=_forced(), repetition_penalty=1.2, presence_penalty=0.5, frequency_penalty=0.5,
               logit_bias={3: 1.0}, penalty_context_ids=[[1], [2]], penalty_context_room=4, penalty_history=8,
               row_sampling=[_params(), _params()], row_streams=[0, 1], row_penalties=True, top_k=5, top_p=0.9, min_p=0.1, top_logprobs=2,
               constraint=_automaton(), constraint_states=[0, 0])
    for name, value in off.items():
        cases[f"speculative greedy with {name}"] = functools.partial(S, "speculative context", **{name: value})
        cases[f"speculative sampled with {name}"] = functools.partial(S, "speculative sampled", **{name: value})
    for name, env, arm in (("UMV_DECODE_SPLITK=9", {"UMV_DECODE_SPLITK": "9"}, "greedy"),
                           ("split-K above 128 rows", {"UMV_DECODE_SPLITK": "3,4,4"}, "greedy B=129"),
                           ("speculative with UMV_DECODE_FUSED_ARGMAX=0", {"UMV_DECODE_FUSED_ARGMAX": "0"}, "speculative context")):
        def run(env=env, arm=arm):
            with _env(env):
                S(arm)
        cases[name] = run
    out = {}
    for name, call in cases.items():
        try:
            call()
            out[name] = "accepted"
        except Exception as e:      # noqa: BLE001 - the type and the text are the record
            out[name] = f"{type(e).__name__}: {e}"
    return out


@functools.lru_cache(maxsize=None)
def _table():
    """everything this module records, of the imported unimedvl_amd"""
    calls = []
    with _seams(calls) as ops, _env({}):
        cases = {arm: _case(ops, calls, arm) for arm in ARMS}
        states = {arm: _states(ops, arm) for arm in STATE_ARMS}
        refusals = _refusals(ops)
    return dict(cases=cases, states=states, refusals=refusals)


def _pack(table):
    """the golden's form: every distinct string once, cases and states as indices"""
    strings, index = [], {}

    def ref(s):
        if s not in index:
            index[s] = len(strings)
            strings.append(s)
        return index[s]
    cases = {arm: dict(ctor=[ref(s) for s in c["ctor"]], step=[ref(s) for s in c["step"]], plan=ref(json.dumps(c["plan"], sort_keys=True)))
             for arm, c in table["cases"].items()}
    states = {arm: {when: ref(json.dumps(v, sort_keys=True)) for when, v in by_when.items()} for arm, by_when in table["states"].items()}
    return dict(strings=strings, cases=cases, states=states, refusals=table["refusals"])


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_step_calls_as_in_the_parent():
    """constructor calls, the first step's calls, and what the session decided and allocated (the plan), arm by arm"""
    g, got = _golden(), _table()["cases"]
    assert sorted(got) == sorted(g["cases"]), "the arms of this module and of the recorded table differ: record again from the parent"
    for arm, c in got.items():
        want = g["cases"][arm]
        for part in ("ctor", "step"):
            parent = [g["strings"][i] for i in want[part]]
            assert not any("?" in s for s in c[part]), f"{arm}: a pointer of its {part} calls resolves to nothing\n  " + "\n  ".join(c[part])
            assert c[part] == parent, f"{arm} {part}\n  now:    " + "\n          ".join(c[part]) + "\n  parent: " + "\n          ".join(parent)
        assert c["plan"] == json.loads(g["strings"][want["plan"]]), arm


def test_a_second_step_records_the_same_calls():
    for arm, c in _table()["cases"].items():
        assert c["step2"] == c["step"], arm


def test_host_written_state_as_in_the_parent():
    """_state(), pen_bias and row_table after construction, set_slot, rewind_outputs and the copy_* methods"""
    g, got = _golden(), _table()["states"]
    assert sorted(got) == sorted(g["states"])
    for arm, by_when in got.items():
        assert list(by_when) == list(g["states"][arm])
        for when, v in by_when.items():
            assert json.loads(json.dumps(v)) == json.loads(g["strings"][g["states"][arm][when]]), f"{arm} after {when}"


def test_refusals_as_in_the_parent():
    g, got = _golden()["refusals"], _table()["refusals"]
    assert sorted(got) == sorted(g)
    for name in got:
        assert got[name] == g[name], name


def _host_cost():
    """microseconds per un-captured _step() of four arms (a session without a graph - tests, tools - pays this per token)"""
    with _seams(None) as ops, _env({}):
        arms = {"greedy": _session(ops, "greedy"),
                "sampled+penalised+constrained": _session(ops, "constraint sampled penalties"),
                "rows+top-n": _session(ops, "top_logprobs rows"),
                "sampled speculative": _session(ops, "speculative sampled")}
        for name, sess in arms.items():
            reps = sorted(timeit.timeit(sess._step, number=2000) / 2000 * 1e6 for _ in range(5))
            print(f"{name:30s} us/step, 2000 steps x 5 repeats: {' '.join(f'{r:.1f}' for r in reps)}   median {reps[2]:.1f}  slowest {reps[4]:.1f}")


if __name__ == "__main__":
    sys.path.append(os.path.dirname(HERE))      # behind PYTHONPATH: a parent checkout named there wins
    import unimedvl_amd
    if "--host-cost" in sys.argv:
        print(f"unimedvl_amd from {os.path.dirname(unimedvl_amd.__file__)}")
        _host_cost()
    elif "--record" in sys.argv:
        if os.path.realpath(os.path.dirname(unimedvl_amd.__file__)).startswith(os.path.realpath(os.path.dirname(HERE)) + os.sep):
            sys.exit("--record takes unimedvl_amd from a checkout of the PARENT commit on PYTHONPATH, never from this tree")
        packed = _pack(_table())
        with open(GOLDEN, "w") as f:
            json.dump(packed, f, indent=0)
            f.write("\n")
        print(f"{len(packed['cases'])} arms, {len(packed['strings'])} strings -> {GOLDEN}")
