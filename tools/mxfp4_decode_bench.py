#!/usr/bin/env python
"""MXFP4 decode weights (llm_weight_dtype = "fp4") against bf16 and e4m3 on the MI355X, two measurements in one process:

  gemm  the four decode GEMMs of the 14B model at M = 8 and 32 rows, in the form the decode step calls them (QKV / o / down as
        3 / 4 / 4-way split-K partials, gate_up with the SwiGLU epilogue), bf16 / e4m3 / MXFP4 alternated shape by shape; COLD
        weights (rotating through > 600 MB of distinct copies, nothing resident in the 256 MiB memory-side cache).  Reported:
        us per call and the algorithmic bytes (weight image incl. scales + x + output) / time as a fraction of 8 TB/s.
  step  ms per greedy decode step (graph replay) at the full 14B dimensions, random weights, B = 8, 1060 tokens of context per
        sample (448 x 448 image + prompt, the headline run's), for the three weight types in the same process, alternated
        REPEATS times; the spread over the repeats is reported.

    python tools/mxfp4_decode_bench.py [--steps 64] [--warmup 8] [--repeats 3] [--out FILE]
UMV_MXFP4_NP = 1 | 2 | 4 fixes the tile pairs per workgroup of the MXFP4 kernel (the sweep of the policy in gemm_mxfp4.hip)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from unimedvl_amd import ops  # noqa: E402

H, I, QKV = 3584, 18944, 4608
BF16 = torch.bfloat16
PEAK = 8e12
MODES = ("bf16", "fp8", "fp4")


def _timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _image_bytes(lin, mode):
    if mode == "fp4":
        return lin.w4.numel()
    if mode == "fp8":
        return lin.w8.numel() + 4 * lin.scale.numel()
    return lin.wp.numel() * 2


def _make(mode, N, K, swiglu, g):
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).to(BF16)
    if swiglu:
        gate, up = w[:N // 2].contiguous(), w[N // 2:].contiguous()
        lin = {"bf16": ops.PackedLinear.from_gate_up, "fp8": ops.PackedLinear.from_gate_up_fp8,
               "fp4": ops.PackedLinear.from_gate_up_mxfp4}[mode](gate, up)
    else:
        lin = {"bf16": ops.PackedLinear.from_weight, "fp8": ops.PackedLinear.from_weight_fp8,
               "fp4": ops.PackedLinear.from_weight_mxfp4}[mode](w)
    if mode != "bf16":
        lin.wp = None          # the M <= 64 kernels stream only the quantised image
    return lin


def gemm_leg(rows_list=(8, 32), reps=200):
    shapes = [("qkv", QKV, H, False, 3), ("o", H, H, False, 4), ("gate_up", 2 * I, H, True, 1), ("down", H, I, False, 4)]
    out = []
    g = torch.Generator(device="cuda").manual_seed(7)
    for name, N, K, swiglu, S in shapes:
        lins = {}
        for mode in MODES:
            one = _make(mode, N, K, swiglu, g)
            nb = _image_bytes(one, mode)
            lins[mode] = [one] + [_make(mode, N, K, swiglu, g) for _ in range(max(2, int(600e6 // nb)))]
        for M in rows_list:
            x = torch.randn(M, K, device="cuda", generator=g).to(BF16)
            res = {}
            for mode in MODES:           # alternated: one shape, the three weight types back to back
                ls = lins[mode]
                if S > 1:
                    p = torch.empty((S, M, N), dtype=torch.float32, device="cuda")
                    fn = lambda i, ls=ls, p=p: ops.gemm_splitk(x, ls[i % len(ls)], p, S)   # noqa: E731
                    obytes = S * M * N * 4
                else:
                    o = torch.empty((M, N // 2 if swiglu else N), dtype=BF16, device="cuda")
                    fn = lambda i, ls=ls, o=o: ops.gemm(x, ls[i % len(ls)], out=o)         # noqa: E731
                    obytes = o.numel() * 2
                fn(0)
                us = _timed(fn, reps)
                nbytes = _image_bytes(ls[0], mode) + M * K * 2 + obytes
                res[mode] = dict(us=round(us, 2), gbps=round(nbytes / us * 1e-3, 1), frac_of_8TBps=round(nbytes / (us * 1e-6) / PEAK, 3),
                                 weight_bytes=_image_bytes(ls[0], mode))
            out.append(dict(gemm=name, N=N, K=K, M=M, k_splits=S, **{m: res[m] for m in MODES}))
            print(json.dumps(out[-1]), flush=True)
        del lins
        torch.cuda.empty_cache()
    return out


def step_leg(B=8, ctx=1060, steps=64, warmup=8, repeats=3):
    from unimedvl_amd.config import UniMedVLConfig
    from unimedvl_amd.decode import DecodeSession
    from unimedvl_amd.kvcache import NaiveCache
    from unimedvl_amd.llm import Qwen2MoT
    from unimedvl_amd.weights import LLMWeights, random_getter
    dev = "cuda"
    sessions, wbytes = {}, {}
    for mode in MODES:
        cfg = UniMedVLConfig()
        cfg.llm_weight_dtype = mode
        llm = Qwen2MoT(cfg, LLMWeights(cfg, random_getter(cfg, dev, seed=1234), dev, load_gen=False), dev)
        cache = NaiveCache(cfg.layers)
        total = warmup + repeats * steps
        cache.ensure(B, ctx + total + 8, cfg.kv_heads, cfg.head_dim, dev)
        cache.lens = [ctx] * B           # a context of zero keys / values (KVSlab allocates zeros): timing depends on lengths only
        start = torch.randint(1000, 100000, (B,), generator=torch.Generator().manual_seed(5))
        sess = DecodeSession(llm, cache, start, torch.full((B,), ctx, dtype=torch.int64), total + 1, use_graph=True)
        sess.step(warmup)
        sessions[mode], wbytes[mode] = sess, llm.w.decode_weight_bytes()
    torch.cuda.synchronize()
    times = {m: [] for m in MODES}
    for _ in range(repeats):
        for mode in MODES:
            times[mode].append(_timed(lambda i, s=sessions[mode]: s.step(1), steps) * 1e-3)
    out = {}
    for mode in MODES:
        t = times[mode]
        out[mode] = dict(ms_per_step=round(statistics.median(t), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4),
                         all_ms=[round(v, 4) for v in t], tokens_per_s=round(B / (statistics.median(t) * 1e-3), 1),
                         weight_bytes_per_step=int(wbytes[mode]))
    res = dict(B=B, context=ctx, steps=steps, repeats=repeats, decode="hipGraph", **out)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--legs", default="gemm,step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mxfp4_decode_bench needs a GPU")
    legs = args.legs.split(",")
    res = dict(device=torch.cuda.get_device_name(0), mxfp4_np=os.environ.get("UMV_MXFP4_NP", "policy"))
    if "gemm" in legs:
        res["gemm"] = gemm_leg()
    if "step" in legs:
        res["step"] = step_leg(steps=args.steps, warmup=args.warmup, repeats=args.repeats)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
