#!/usr/bin/env python
"""The tiled GEMM on the MXFP4 image (umv_gemm_mxfp4t, M > 64) and the fp4 mode without bf16 images (llm_fp4_keep_bf16=False) on the
MI355X, three measurements in one process:

  step      ms per greedy decode step (graph replay) at 96 and 128 samples, full 14B dimensions, random weights, 1060 tokens of context
            per sample: standalone fp4 (65..128 rows stream the MXFP4 images through umv_gemm_mxfp4t) against carried fp4 (the same rows
            stream the bf16 images of W' through umv_gemm_bf16 - the behaviour before the kernel existed), alternated REPEATS times; the
            min-max spread of each arm over its repeats is reported, and whether standalone wins by more than the carried arm's spread.
  gemm      us per call of the four model GEMMs at M = 272, 2048 and 8480 rows, in the form prefill calls them (gate_up with the SwiGLU
            epilogue): the MXFP4 image on the tiled kernel against umv_gemm_bf16 on the bf16 image of the same W', sustained loops,
            alternated REPEATS times; ratio and the bf16 arm's spread.
  resident  torch.cuda.memory_allocated() after loading the whole engine (both experts, ViT, lm_head) in standalone fp4 mode.

    python tools/mxfp4_tiled_bench.py [--steps 48] [--warmup 8] [--repeats 3] [--legs step,gemm,resident] [--out FILE]
UMV_MXFP4T_NP = 1 | 2 fixes the tile pairs per wave of the kernel (A/B of the policy in gemm_mxfp4t.hip)."""
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


def _timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _summary(t):
    return dict(median=round(statistics.median(t), 3), min=round(min(t), 3), max=round(max(t), 3), all=[round(v, 3) for v in t])


def step_leg(batches=(96, 128), ctx=1060, steps=48, warmup=8, repeats=3):
    from unimedvl_amd.config import UniMedVLConfig
    from unimedvl_amd.decode import DecodeSession
    from unimedvl_amd.kvcache import NaiveCache
    from unimedvl_amd.llm import Qwen2MoT
    from unimedvl_amd.weights import LLMWeights, random_getter
    dev = "cuda"
    llms = {}
    for arm, keep in (("carried", True), ("standalone", False)):
        cfg = UniMedVLConfig()
        cfg.llm_weight_dtype = "fp4"
        cfg.llm_fp4_keep_bf16 = keep
        llms[arm] = Qwen2MoT(cfg, LLMWeights(cfg, random_getter(cfg, dev, seed=1234), dev, load_gen=False), dev)
    out = []
    for B in batches:
        sessions = {}
        total = warmup + repeats * steps
        for arm, llm in llms.items():
            cfg = llm.cfg
            cache = NaiveCache(cfg.layers)
            cache.ensure(B, ctx + total + 8, cfg.kv_heads, cfg.head_dim, dev)
            cache.lens = [ctx] * B           # a context of zero keys / values: timing depends on lengths only
            start = torch.randint(1000, 100000, (B,), generator=torch.Generator().manual_seed(5))
            sess = DecodeSession(llm, cache, start, torch.full((B,), ctx, dtype=torch.int64), total + 1, use_graph=True)
            sess.step(warmup)
            sessions[arm] = sess
        torch.cuda.synchronize()
        times = {a: [] for a in sessions}
        for _ in range(repeats):
            for arm in ("carried", "standalone"):
                times[arm].append(_timed(lambda i, s=sessions[arm]: s.step(1), steps) * 1e-3)
        same = torch.equal(sessions["carried"].in_ids[:total], sessions["standalone"].in_ids[:total])
        c, s = _summary(times["carried"]), _summary(times["standalone"])
        spread = c["max"] - c["min"]
        row = dict(B=B, context=ctx, steps=steps, repeats=repeats, decode="hipGraph", splitk=list(sessions["standalone"].sk),
                   carried_ms=c, standalone_ms=s, gain_ms=round(c["median"] - s["median"], 3), carried_spread_ms=round(spread, 3),
                   faster_beyond_spread=bool(c["min"] - s["max"] > spread), same_tokens=bool(same),
                   tokens_per_s=dict(carried=round(B / (c["median"] * 1e-3), 1), standalone=round(B / (s["median"] * 1e-3), 1)))
        print(json.dumps(row), flush=True)
        out.append(row)
        del sessions
        torch.cuda.empty_cache()
    return out


def gemm_leg(rows_list=(272, 2048, 8480), repeats=3, window_ms=60.0):
    shapes = [("qkv", QKV, H, False), ("o", H, H, False), ("gate_up", 2 * I, H, True), ("down", H, I, False)]
    out = []
    g = torch.Generator(device="cuda").manual_seed(7)
    for name, N, K, swiglu in shapes:
        w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).to(BF16)
        if swiglu:
            full = ops.PackedLinear.from_gate_up_mxfp4(w[:N // 2].contiguous(), w[N // 2:].contiguous())
        else:
            full = ops.PackedLinear.from_weight_mxfp4(w)
        del w
        arms = dict(bf16=ops.PackedLinear(full.wp, None, N, K, swiglu=swiglu), fp4=ops.PackedLinear(None, None, N, K, swiglu=swiglu, w4=full.w4))
        for M in rows_list:
            x = torch.randn(M, K, device="cuda", generator=g).to(BF16)
            o = {a: torch.empty((M, N // 2 if swiglu else N), dtype=BF16, device="cuda") for a in arms}
            fns = {a: (lambda i, a=a: ops.gemm(x, arms[a], out=o[a])) for a in arms}
            reps = {}
            for a in arms:
                fns[a](0)
                reps[a] = max(20, int(window_ms * 1e3 / max(_timed(fns[a], 10), 1.0)))
            t = {a: [] for a in arms}
            for _ in range(repeats):
                for a in ("bf16", "fp4"):
                    t[a].append(_timed(fns[a], reps[a]))
            b, f = _summary(t["bf16"]), _summary(t["fp4"])
            flops = 2.0 * M * N * K
            row = dict(gemm=name, M=M, N=N, K=K, bf16_us=b, fp4_us=f, ratio_fp4_over_bf16=round(f["median"] / b["median"], 3),
                       bf16_spread=round((b["max"] - b["min"]) / b["median"], 3), tflops=dict(bf16=round(flops / b["median"] * 1e-6, 1),
                                                                                                 fp4=round(flops / f["median"] * 1e-6, 1)),
                       bit_identical=bool(torch.equal(o["bf16"], o["fp4"])))
            print(json.dumps(row), flush=True)
            out.append(row)
        del arms, full
        torch.cuda.empty_cache()
    return out


def resident_leg():
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.config import UniMedVLConfig
    from unimedvl_amd.weights import random_getter
    out = {}
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    cfg = UniMedVLConfig()
    cfg.llm_weight_dtype = "fp4"
    cfg.llm_fp4_keep_bf16 = False
    model = Bagel(cfg, random_getter(cfg, "cuda", seed=1234), device="cuda")
    torch.cuda.synchronize()
    out["standalone_fp4"] = dict(resident_bytes=int(torch.cuda.memory_allocated() - base),
                                 peak_during_load_bytes=int(torch.cuda.max_memory_allocated() - base),
                                 decode_weight_bytes_per_step=int(model.language_model.w.decode_weight_bytes()))
    del model
    torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--legs", default="step,gemm,resident")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mxfp4_tiled_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mxfp4_tiled_bench needs a GPU")
    legs = args.legs.split(",")
    res = dict(device=torch.cuda.get_device_name(0), mxfp4t_np=os.environ.get("UMV_MXFP4T_NP", "policy"))
    if "gemm" in legs:
        res["gemm"] = gemm_leg(repeats=args.repeats)
    if "step" in legs:
        res["step"] = step_leg(steps=args.steps, warmup=args.warmup, repeats=args.repeats)
    if "resident" in legs:
        res["resident"] = resident_leg()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
