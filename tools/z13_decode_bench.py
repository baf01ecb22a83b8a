#!/usr/bin/env python
"""The exact 13-bit decode images (llm_decode_z13) against the bf16 images they restate, on the MI355X, in one process:

  gemm  the decode GEMMs of the 14B model at M = 8, 16 and 32 rows in the form the decode step calls them (QKV / o / down as 3 / 4 / 4-way
        split-K partials, gate_up with the SwiGLU epilogue, lm_head with the argmax keys), bf16 against z13 on the SAME weights,
        alternated shape by shape, COLD (rotating through > 600 MB of distinct copies, nothing resident in the 256 MiB memory-side
        cache: tools/skinny_bench.py's method).  Reported: us per call, TB/s of the weight bytes actually read, flagged blocks.
  step  ms per greedy decode step (graph replay) at the full 14B dimensions, random weights, B = 8 at 1060 tokens of context (the
        headline run's) and B = 32 at 1156: the images off (the path before them: the same PackedLinear objects without the image)
        and on, alternated REPEATS times on one set of weights; min - max per arm.

  pmc   only the gate/up GEMM at 8 rows, both arms: what tools/z13_pmc.sh runs under `rocprofv3 --pmc`.

    python tools/z13_decode_bench.py [--steps 64] [--warmup 8] [--repeats 3] [--legs gemm,step] [--out FILE]"""
import argparse
import copy
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from unimedvl_amd import ops  # noqa: E402

H, I, QKV, V = 3584, 18944, 4608, 152064
BF16 = torch.bfloat16
ARMS = ("bf16", "z13")


def _timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _twin(lin):
    return ops.PackedLinear(lin.wp, lin.bias, lin.N, lin.K, swiglu=lin.swiglu, th=lin.th)


def _flagged_share(lin):
    NP = ((lin.N + 15) // 16 + 1) // 2
    flags = lin.wz[:16 * NP].cpu().numpy().view("uint64")[0::2]          # 16-byte head entries: flags u64, base, zeros
    blocks = NP * ((lin.K + 511) // 512)
    return sum(bin(int(f)).count("1") for f in flags) / blocks


def _make(N, K, swiglu, g):
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).to(BF16)
    lin = ops.PackedLinear.from_gate_up(w[:N // 2].contiguous(), w[N // 2:].contiguous()) if swiglu else ops.PackedLinear.from_weight(w)
    return lin.build_z13()


def gemm_leg(rows_list=(8, 16, 32), reps=200):
    shapes = [("qkv", QKV, H, False, 3), ("o", H, H, False, 4), ("gate_up", 2 * I, H, True, 1), ("down", H, I, False, 4),
              ("lm_head", V, H, False, 1)]
    out = []
    g = torch.Generator(device="cuda").manual_seed(7)
    for name, N, K, swiglu, S in shapes:
        z = [_make(N, K, swiglu, g) for _ in range(max(3, int(600e6 // (N * K * 13 // 8)) + 1))]
        lins = {"z13": z, "bf16": [_twin(l) for l in z]}
        wbytes = {"z13": z[0].wz.numel(), "bf16": z[0].wp.numel() * 2}
        share = _flagged_share(z[0])
        for M in rows_list:
            x = torch.randn(M, K, device="cuda", generator=g).to(BF16)
            res = {}
            for rep in range(2):             # alternated twice: the second pass is reported, the first shows the drift
                for arm in ARMS:
                    ls = lins[arm]
                    if S > 1:
                        p = torch.empty((S, M, N), dtype=torch.float32, device="cuda")
                        fn = lambda i, ls=ls, p=p: ops.gemm_splitk(x, ls[i % len(ls)], p, S)   # noqa: E731
                    elif name == "lm_head":
                        o = torch.empty((M, N), dtype=BF16, device="cuda")
                        keys = torch.zeros((M, (N + 15) // 16), dtype=torch.int64, device="cuda")
                        fn = lambda i, ls=ls, o=o, keys=keys: ops.gemm(x, ls[i % len(ls)], out=o, argmax_partial=keys)   # noqa: E731
                    else:
                        o = torch.empty((M, N // 2 if swiglu else N), dtype=BF16, device="cuda")
                        fn = lambda i, ls=ls, o=o: ops.gemm(x, ls[i % len(ls)], out=o)         # noqa: E731
                    fn(0)
                    us = _timed(fn, max(reps // (8 if name == "lm_head" else 1), 3 * len(ls)))
                    res.setdefault(arm, []).append(round(us, 2))
            row = dict(gemm=name, N=N, K=K, M=M, k_splits=S, copies=len(z), flagged_block_share=round(share, 5))
            for arm in ARMS:
                us = res[arm][-1]
                row[arm] = dict(us=us, us_first_pass=res[arm][0], weight_bytes=wbytes[arm], TBps_of_weight_bytes=round(wbytes[arm] / us * 1e-6, 2))
            out.append(row)
            print(json.dumps(row), flush=True)
        del lins, z
        torch.cuda.empty_cache()
    return out


def pmc_leg(reps=30):
    """the gate/up GEMM at 8 rows, z13 then bf16, cold weights: the workload of a counter pass (tools/z13_pmc.sh)"""
    g = torch.Generator(device="cuda").manual_seed(7)
    z = [_make(2 * I, H, True, g) for _ in range(3)]
    x = torch.randn(8, H, device="cuda", generator=g).to(BF16)
    o = torch.empty((8, I), dtype=BF16, device="cuda")
    for ls in (z, [_twin(l) for l in z]):
        for i in range(reps):
            ops.gemm(x, ls[i % 3], out=o)
    torch.cuda.synchronize()


def _without_z13(w):
    """the same weights as the engine held them before the images: every linear without its 13-bit image"""
    from unimedvl_amd.weights import LayerWeights
    off = copy.copy(w)
    off.z13 = False
    off.lm_head = _twin(w.lm_head)
    off.und = []
    for lw in w.und:
        c = LayerWeights()
        for f in LayerWeights.__slots__:
            v = getattr(lw, f)
            setattr(c, f, _twin(v) if isinstance(v, ops.PackedLinear) else v)
        off.und.append(c)
    return off


def step_leg(w_on, B, ctx, steps=64, warmup=8, repeats=3):
    from unimedvl_amd.config import UniMedVLConfig
    from unimedvl_amd.decode import DecodeSession
    from unimedvl_amd.kvcache import NaiveCache
    from unimedvl_amd.llm import Qwen2MoT
    dev = "cuda"
    cfg = UniMedVLConfig()
    sessions, wbytes = {}, {}
    for arm, w in (("bf16", _without_z13(w_on)), ("z13", w_on)):
        llm = Qwen2MoT(cfg, w, dev)
        cache = NaiveCache(cfg.layers)
        total = warmup + repeats * steps
        cache.ensure(B, ctx + total + 8, cfg.kv_heads, cfg.head_dim, dev)
        cache.lens = [ctx] * B           # a context of zero keys / values (KVSlab allocates zeros): timing depends on lengths only
        start = torch.randint(1000, 100000, (B,), generator=torch.Generator().manual_seed(5))
        sess = DecodeSession(llm, cache, start, torch.full((B,), ctx, dtype=torch.int64), total + 1, use_graph=True)
        sess.step(warmup)
        sessions[arm], wbytes[arm] = sess, w.decode_weight_bytes()
    torch.cuda.synchronize()
    times = {a: [] for a in ARMS}
    for _ in range(repeats):
        for arm in ARMS:
            times[arm].append(_timed(lambda i, s=sessions[arm]: s.step(1), steps) * 1e-3)
    same = torch.equal(sessions["bf16"].pred_ids[:warmup + repeats * steps], sessions["z13"].pred_ids[:warmup + repeats * steps])
    out = {}
    for arm in ARMS:
        t = times[arm]
        out[arm] = dict(ms_per_step=round(statistics.median(t), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4),
                        all_ms=[round(v, 4) for v in t], tokens_per_s=round(B / (statistics.median(t) * 1e-3), 1),
                        weight_bytes_per_step=int(wbytes[arm]))
    spread = out["bf16"]["max_ms"] - out["bf16"]["min_ms"]
    res = dict(B=B, context=ctx, steps=steps, repeats=repeats, decode="hipGraph", same_token_ids=bool(same),
               gain_ms=round(out["bf16"]["ms_per_step"] - out["z13"]["ms_per_step"], 4), bf16_spread_ms=round(spread, 4), **out)
    print(json.dumps(res), flush=True)
    del sessions
    torch.cuda.empty_cache()
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
        raise SystemExit("z13_decode_bench needs a GPU")
    legs = args.legs.split(",")
    res = dict(device=torch.cuda.get_device_name(0))
    if "pmc" in legs:
        return pmc_leg()
    if "gemm" in legs:
        res["gemm"] = gemm_leg()
    if "step" in legs:
        from unimedvl_amd.config import UniMedVLConfig
        from unimedvl_amd.weights import LLMWeights, random_getter
        cfg = UniMedVLConfig()
        cfg.llm_decode_z13 = True
        w = LLMWeights(cfg, random_getter(cfg, "cuda", seed=1234), "cuda", load_gen=False)
        lins = [w.lm_head] + [l for lw in w.und for l in (lw.gate_up, lw.down)]
        res["flagged_block_share"] = round(sum(_flagged_share(l) for l in lins) / len(lins), 6)
        res["z13_resident_bytes"] = int(sum(l.wz.numel() for l in lins))
        res["step"] = [step_leg(w, 8, 1060, args.steps, args.warmup, args.repeats),
                       step_leg(w, 32, 1156, args.steps, args.warmup, args.repeats)]
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
