"""Which weight image and which C entry point serve a GEMM call (ops.gemm / ops.gemm_splitk), pinned call by call against a table
recorded from the PARENT of the commit that folded the routing into ops._route - never from the tree under test.

The routing layer runs without a GPU or the shared library behind three seams: _lib.load returns a recorder (every attribute a function
that logs (name, args) and returns 0), ops._stream returns None, ops._req checks the dtype only.  CPU tensors then flow through
unchanged.  A recorded call is normalised: argument structures are expanded field by field (fields left at zero are omitted), every
pointer becomes the name of the tensor it points to (x, out, residual, row_idx, norm_w, argmax_partial, step, lin.<image>, lin.bias,
or tmp<k> for the k-th tensor allocated inside the call), the row count becomes M, and an exception is its type and message.

    python tests/test_gemm_routing_cpu.py --record      with PYTHONPATH = a checkout of the parent commit (git worktree add DIR <parent>):
                                                        rewrites tests/golden/gemm_routing.json; refuses to record from this tree
    python tests/test_gemm_routing_cpu.py --host-cost   microseconds per ops.gemm call under the recorder (profiles/gemm_routing_refactor.txt)
"""
import ctypes as C
import functools
import json
import os
import sys
import timeit

import torch

from abi_recorder import _seams, render

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gemm_routing.json")
BF16 = torch.bfloat16
N, K = 64, 128
MS = (1, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129)       # both sides of every row boundary of the policy, and of umv_gemm_bf16's split-K limit
KINDS = ("bf16", "bf16_th8", "bf16_z13", "fp8", "fp8_mfma", "fp8_mfma_only", "fp4", "fp4_only")
VARIANTS = ("plain", "bias", "swiglu")
FORMS = ("plain", "no_bias", "residual", "gelu_tanh", "silu", "out_f32", "row_idx", "norm_w", "argmax", "argmax_sample", "act8", "splitk")
IMAGES = ("wp", "w8", "scale", "w8m", "w4", "wz", "bias")
M_ARG = {"umv_quantize_act_fp8": 8}       # the position of the row count among the plain arguments of a recorded function


def _linear(ops, kind, variant):
    u8 = lambda: torch.empty(N * K, dtype=torch.uint8)      # noqa: E731
    lin = ops.PackedLinear(torch.empty(N * K, dtype=BF16), torch.empty(N, dtype=BF16) if variant == "bias" else None, N, K,
                           swiglu=variant == "swiglu", th=8 if kind == "bf16_th8" else 16)
    if kind.startswith("fp8"):
        lin.w8, lin.scale = u8(), torch.empty(N, dtype=torch.float32)
    if kind.startswith("fp8_mfma"):
        lin.w8m = u8()
    if kind.startswith("fp4"):
        lin.w4 = u8()
    if kind == "bf16_z13":
        lin.wz = u8()
    if kind.endswith("_only"):
        lin.wp = None
    return lin


def _linears():
    for kind in KINDS:
        for variant in VARIANTS:
            if not (kind == "bf16_th8" and variant == "swiglu"):        # th-row tiles are a layout without SwiGLU (for_decode)
                yield kind, variant


def _cases():
    for kind, variant in _linears():
        for form in FORMS:
            for z13 in ((None, True, False) if kind == "bf16_z13" else (None,)):
                yield kind, variant, form, z13


def _run(ops, lin, form, z13, M):
    """one call; returns the tensors it was given, by name"""
    n_out = N // 2 if lin.swiglu else N
    t = {"x": torch.empty((M, K), dtype=BF16)}
    kw = {}
    if form == "splitk":
        t["out"] = torch.empty((2, M, N), dtype=torch.float32)
        return t, lambda: ops.gemm_splitk(t["x"], lin, t["out"], 2, z13=z13)
    if form == "no_bias":
        kw["use_bias"] = False
    elif form == "residual":
        t["residual"] = kw["residual"] = torch.empty((M, n_out), dtype=BF16)
    elif form in ("gelu_tanh", "silu"):
        kw["act"] = form
    elif form == "out_f32":
        kw["out_f32"] = True
    elif form == "row_idx":     # M rows of a larger buffer
        t["x"] = torch.empty((M + 3, K), dtype=BF16)
        t["row_idx"] = kw["row_idx"] = torch.arange(M, dtype=torch.int32)
        t["out"] = kw["out"] = torch.empty((M + 3, n_out), dtype=BF16)
        kw["M"] = M
    elif form == "norm_w":
        t["norm_w"] = kw["norm_w"] = torch.empty(K, dtype=BF16)
    elif form in ("argmax", "argmax_sample"):
        t["argmax_partial"] = kw["argmax_partial"] = torch.empty((M, (N + 15) // 16), dtype=torch.int64)
        if form == "argmax_sample":
            t["step"] = torch.zeros(1, dtype=torch.int64)
            kw["sample"] = (0.75, 1234, t["step"])
    elif form == "act8":
        kw["act8"] = True
    return t, lambda: ops.gemm(t["x"], lin, z13=z13, **kw)


def _record(ops, calls, made, kind, variant, form, z13, M):
    """the normalised record of one case: "fn(args) ; fn(args) ; ..." with a raised exception as the last item"""
    lin = _linear(ops, kind, variant)
    del calls[:], made[:]
    given, call = _run(ops, lin, form, z13, M)
    try:
        call()
        raised = []
    except Exception as e:      # noqa: BLE001 - the type and the text are the record
        raised = [f"{type(e).__name__}: {e}".replace(f"M={M} rows", "M=<M> rows")]
    names = {t.data_ptr(): name for name, t in given.items()}
    names.update({getattr(lin, f).data_ptr(): "lin." + f for f in IMAGES if getattr(lin, f) is not None})
    tmp = [t for t in made if t.data_ptr() not in names]
    names.update({t.data_ptr(): f"tmp{k}" for k, t in enumerate(tmp)})

    def ptr(v):
        v = v.value if isinstance(v, C.c_void_p) else v
        return "0" if v is None else names.get(v, "?")

    def rows(v):
        return "M" if v == M else f"M+{v - M}"

    def field(f, fv):
        if f == "split_stride" and fv % M == 0:
            return f"M*{fv // M}"
        return rows(fv) if f in ("M", "x_rows") else fv

    items = render(calls, ptr, lambda v: v in names, field, lambda fn, i, v: rows(v) if M_ARG.get(fn) == i else str(v))
    return " ; ".join(items + raised)


@functools.lru_cache(maxsize=None)
def _table():
    """{case: {record: [M, ...]}} of the imported unimedvl_amd, and the answers of ops._z13_takes"""
    calls, made, table = [], [], {}
    with _seams(calls, made) as ops:
        for kind, variant, form, z13 in _cases():
            by_record = table.setdefault(f"{kind}/{variant} {form} z13={z13}", {})
            for M in MS:
                by_record.setdefault(_record(ops, calls, made, kind, variant, form, z13, M), []).append(M)
        lin = _linear(ops, "bf16_z13", "plain")
        takes = {f"{form} z13={z13}": "".join(str(int(ops._z13_takes(lin, M, z13, form))) for M in range(1, 66))
                 for form in ("splitk", "epilogue", None) for z13 in (None, True, False)}
    return table, takes


def _constructors():
    """{constructor call: its library calls and the linear it returns}: the from_* constructors of PackedLinear"""
    calls, made, table = [], [], {}
    with _seams(calls, made) as ops:
        P = ops.PackedLinear
        for name, keep in (("from_weight", None), ("from_gate_up", None), ("from_weight_fp8", None), ("from_gate_up_fp8", None),
                           ("from_weight_mxfp4", True), ("from_weight_mxfp4", False), ("from_gate_up_mxfp4", True), ("from_gate_up_mxfp4", False)):
            for with_bias in ((False, True) if "weight" in name else (False,)):
                given = {"w": torch.empty((N, K), dtype=BF16), "up": torch.empty((N, K), dtype=BF16), "bias": torch.empty(N, dtype=BF16)}
                take = ("w", "up") if "gate_up" in name else ("w", "bias") if with_bias else ("w",)
                del calls[:], made[:]
                lin = getattr(P, name)(*(given[n] for n in take), **({} if keep is None else {"keep_bf16": keep}))
                names = {t.data_ptr(): n for n, t in given.items()}
                names.update({t.data_ptr(): f"tmp{k}" for k, t in enumerate(made)})
                ptr = lambda v: "0" if v is None or v.value is None else names.get(v.value, "?")      # noqa: E731
                lib = " ; ".join(f"{fn}({', '.join(ptr(v) if v is None or isinstance(v, C.c_void_p) else str(v) for v in a)})" for fn, a in calls)
                held = " ".join(f"{f}={'0' if getattr(lin, f) is None else names.get(getattr(lin, f).data_ptr(), '?')}" for f in IMAGES)
                table[f"{name}({', '.join(take)}{'' if keep is None else f', keep_bf16={keep}'})"] = \
                    f"{lib} -> N={lin.N} K={lin.K} swiglu={lin.swiglu} th={lin.th} {held}"
    return table


class _Store:
    """a pack store (packstore.PackStore's two methods) that builds everything and logs what it was asked for"""
    def __init__(self, log):
        self.log = log

    def linear(self, key, build):
        self.log.append(("store.linear " + key, ()))
        return build()

    def tensor(self, name, build):
        self.log.append(("store.tensor " + name, ()))
        return build()


LOADS = {"bf16": {}, "bf16 without z13": dict(llm_decode_z13=False), "fp8": dict(llm_weight_dtype="fp8"),
         "fp8 W8A8": dict(llm_weight_dtype="fp8", llm_act_dtype="fp8"), "fp4": dict(llm_weight_dtype="fp4"),
         "fp4 alone": dict(llm_weight_dtype="fp4", llm_fp4_keep_bf16=False)}


def _loads():
    """{mode: what LLMWeights asks of the checkpoint, the pack store and the library, in order, and the images every linear ends up with}
    for a one-layer model"""
    from oracle.weights import TINY
    from unimedvl_amd import shapes, weights
    from unimedvl_amd.config import UniMedVLConfig
    table = {}
    for mode, over in LOADS.items():
        cfg = UniMedVLConfig.from_dict(dict(TINY, layers=1))
        for k, v in over.items():
            setattr(cfg, k, v)
        shp, log = shapes.all_shapes(cfg), []

        def get(name):
            log.append(("get " + name, ()))
            return torch.zeros(shp[name], dtype=BF16)
        get.pack_store = _Store(log)
        with _seams(log):
            w = weights.LLMWeights(cfg, get, "cpu")
        held = {"lm_head": w.lm_head, **{f"{e}.{f}": getattr(lw, f) for e, lw in (("und", w.und[0]), ("gen", w.gen[0]))
                                         for f in ("qkv", "o", "gate_up", "down")}}
        table[mode] = " ; ".join(what.replace("language_model.", "") for what, _ in log) + " -> " + " ".join(
            f"{name}={'+'.join(f for f in IMAGES if getattr(lin, f) is not None)}" for name, lin in held.items()) + \
            f" fp8={w.fp8} fp4={w.fp4} act8={w.act8} fp4_keep_bf16={w.fp4_keep_bf16} z13={w.z13}"
    return table


def _lines(table):
    """one line per (case, rows that record alike)"""
    return [f"{case} M={','.join(map(str, ms))} | {rec}" for case, by_record in table.items() for rec, ms in by_record.items()]


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_call_routes_as_in_the_parent():
    table, _ = _table()
    want = {}
    for line in _golden()["calls"]:
        head, rec = line.split(" | ", 1)
        case, ms = head.rsplit(" M=", 1)
        for M in ms.split(","):
            want[case, int(M)] = rec
    got = {(case, M): rec for case, by_record in table.items() for rec, ms in by_record.items() for M in ms}
    assert len(got) == sum(len(MS) for _ in _cases())
    assert sorted(got, key=str) == sorted(want, key=str), "the grid of this module and of the recorded table differ: record again from the parent"
    for key in got:
        assert got[key] == want[key], f"{key[0]} M={key[1]}\n  now:    {got[key]}\n  parent: {want[key]}"


def test_z13_takes_answers_as_in_the_parent():
    _, takes = _table()
    assert takes == _golden()["z13_takes"]
    with _seams(None) as ops:     # no image, no streaming of it, whatever the override
        lin = _linear(ops, "bf16", "plain")
        assert not any(ops._z13_takes(lin, M, z13, form) for M in range(1, 66) for z13 in (None, True, False) for form in ("splitk", "epilogue", None))


def test_constructors_and_weight_load_as_in_the_parent():
    """the from_* constructors of PackedLinear (library calls, their arguments, the images of the result) and LLMWeights per mode (load
    order, pack-store keys, library calls, who ends up with which image)"""
    g = _golden()
    for got, want in ((_constructors(), g["constructors"]), (_loads(), g["loads"])):
        assert list(got) == list(want)
        for case in got:
            assert got[case] == want[case], f"{case}\n  now:    {got[case]}\n  parent: {want[case]}"


def test_decode_weight_bytes_is_the_parents_sum():
    """LLMWeights.decode_weight_bytes() per mode against the parent's formula, written out: every image has its own size here"""
    from unimedvl_amd import ops, weights
    sizes = iter(range(1000, 100000, 7))

    def lin(mode, z13=False):
        u8 = lambda: torch.empty(next(sizes), dtype=torch.uint8)        # noqa: E731
        p = ops.PackedLinear(None if mode == "fp4_only" else torch.empty(next(sizes), dtype=BF16), None, N, K)
        if mode == "fp8":
            p.w8, p.scale, p.w8m = u8(), torch.empty(N, dtype=torch.float32), u8()
        if mode in ("fp4", "fp4_only"):
            p.w4 = u8()
        if z13:
            p.wz = u8()
        return p

    for mode in ("bf16", "bf16_z13", "fp8", "fp4", "fp4_only"):
        w = weights.LLMWeights.__new__(weights.LLMWeights)
        w.fp8, w.fp4 = mode == "fp8", mode.startswith("fp4")
        w.lm_head = lin("fp8" if w.fp8 or w.fp4 else "bf16", z13=mode == "bf16_z13")
        w.und = []
        for _ in range(3):
            lw = weights.LayerWeights()
            lw.qkv, lw.o = lin(mode), lin(mode)                                          # q/k/v and o never have a 13-bit image
            lw.gate_up, lw.down = lin(mode, z13=mode == "bf16_z13"), lin(mode, z13=mode == "bf16_z13")
            w.und.append(lw)
        layer = [p for lw in w.und for p in (lw.qkv, lw.o, lw.gate_up, lw.down)]
        if w.fp8:
            want = w.lm_head.w8.numel() + sum(p.w8.numel() for p in layer)
        elif w.fp4:
            want = w.lm_head.w8.numel() + sum(p.w4.numel() for p in layer)
        else:
            want = sum(p.wz.numel() if p.wz is not None else p.wp.numel() * 2 for p in [w.lm_head] + layer)
        assert w.decode_weight_bytes() == want, mode


def _host_cost():
    """microseconds per call of the four forms whose Python cost matters (prefill and flow passes call ops.gemm outside a graph)"""
    with _seams(None) as ops:
        x = torch.empty((65, K), dtype=BF16)
        out, idx = torch.empty((65, N), dtype=BF16), torch.arange(8, dtype=torch.int32)
        forms = {"plain bf16, M=8": (_linear(ops, "bf16", "bias"), x[:8], dict(out=out[:8])),
                 "row_idx bf16, M=8 of 65": (_linear(ops, "bf16", "bias"), x, dict(out=out, row_idx=idx, M=8)),
                 "MXFP4 alone, M=65": (_linear(ops, "fp4_only", "bias"), x, dict(out=out)),
                 "act8, M=65": (_linear(ops, "fp8_mfma_only", "bias"), x, dict(out=out, act8=True))}
        for name, (lin, xx, kw) in forms.items():
            reps = sorted(timeit.timeit(lambda: ops.gemm(xx, lin, **kw), number=20000) / 20000 * 1e6 for _ in range(5))
            print(f"{name:24s} us/call, 20000 calls x 5 repeats: {' '.join(f'{r:.2f}' for r in reps)}   median {reps[2]:.2f}  slowest {reps[4]:.2f}")


if __name__ == "__main__":
    sys.path.append(os.path.dirname(HERE))      # behind PYTHONPATH: a parent checkout named there wins
    import unimedvl_amd
    if "--host-cost" in sys.argv:
        print(f"unimedvl_amd from {os.path.dirname(unimedvl_amd.__file__)}")
        _host_cost()
    elif "--record" in sys.argv:
        if os.path.realpath(os.path.dirname(unimedvl_amd.__file__)).startswith(os.path.realpath(os.path.dirname(HERE)) + os.sep):
            sys.exit("--record takes unimedvl_amd from a checkout of the PARENT commit on PYTHONPATH, never from this tree")
        table, takes = _table()
        with open(GOLDEN, "w") as f:
            json.dump({"calls": _lines(table), "z13_takes": takes, "constructors": _constructors(), "loads": _loads()}, f, indent=0)
            f.write("\n")
        print(f"{sum(len(MS) for _ in _cases())} calls, {len(_lines(table))} lines -> {GOLDEN}")
