#!/usr/bin/env python
"""What truncated sampling (top-k / top-p / min-p in the decode step) costs on the MI355X, at the full 14B dimensions with random
weights, in one process: ms per sampled decode step (graph replay), B = 8 at 1060 tokens of context (the headline run's), five arms on
the same weights, alternated REPEATS times, min - max per arm:

  a  do_sample as today (the lm_head sampling epilogue + umv_decode_step_end_argmax)
  b  top_p = 0.9          c  top_k = 50          d  top_k = 50, top_p = 0.9, min_p = 0.05   (umv_decode_step_end_truncated)
  e  today's unfused sampler (UMV_DECODE_FUSED_ARGMAX=0 around the session's construction: lm_head -> umv_sample_bf16 -> step end),
     the yardstick a truncated step has to beat to be worth fusing

Random weights give nearly flat logits: arm c drops the untruncated pick on almost every step (the slow branch: a second look at the row,
the worst case), arm b keeps it with probability about 0.9 whatever the logits.  The share of steps on each branch is counted on PROBE
further steps per arm, outside the timing: a step took the fast branch iff its token is the column of the largest lm_head key.

    python tools/truncated_sampling_bench.py [--steps 64] [--warmup 8] [--repeats 3] [--probe 32] [--out profiles/truncated_sampling_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

ARMS = {"a_sample": {}, "b_top_p": dict(top_p=0.9), "c_top_k": dict(top_k=50), "d_all": dict(top_k=50, top_p=0.9, min_p=0.05),
        "e_unfused": {}}
TEMPERATURE, SEED = 1.0, 1234


def _timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(llm, B, ctx, steps, warmup, repeats, probe):
    from unimedvl_amd.decode import DecodeSession
    from unimedvl_amd.kvcache import NaiveCache
    cfg, dev = llm.cfg, llm.device
    total = warmup + repeats * steps + probe
    sessions = {}
    for arm, flt in ARMS.items():
        cache = NaiveCache(cfg.layers)
        cache.ensure(B, ctx + total + 8, cfg.kv_heads, cfg.head_dim, dev)
        cache.lens = [ctx] * B           # a context of zero keys / values: timing depends on lengths only
        start = torch.randint(1000, 100000, (B,), generator=torch.Generator().manual_seed(5))
        saved = os.environ.get("UMV_DECODE_FUSED_ARGMAX")
        if arm == "e_unfused":
            os.environ["UMV_DECODE_FUSED_ARGMAX"] = "0"
        try:
            sessions[arm] = DecodeSession(llm, cache, start, torch.full((B,), ctx, dtype=torch.int64), total + 1, use_graph=True,
                                          do_sample=True, temperature=TEMPERATURE, seed=SEED, **flt)
        finally:
            if arm == "e_unfused":
                if saved is None:
                    del os.environ["UMV_DECODE_FUSED_ARGMAX"]
                else:
                    os.environ["UMV_DECODE_FUSED_ARGMAX"] = saved
        sessions[arm].step(warmup)
    times = {a: [] for a in ARMS}
    for _ in range(repeats):
        for arm in ARMS:
            times[arm].append(_timed(lambda i, s=sessions[arm]: s.step(1), steps))
    out = {}
    for arm, flt in ARMS.items():
        t, s = times[arm], sessions[arm]
        out[arm] = dict(filters=flt, ms_per_step=round(statistics.median(t), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4),
                        all_ms=[round(v, 4) for v in t])
        if s.truncated:
            fast = 0
            for _ in range(probe):
                row = s.steps_done
                s.step(1)
                key = s.amax_part.cpu().numpy().view(np.uint64).max(axis=1)          # the keys are unsigned
                fused = (np.uint64(0xFFFFFFFF) - (key & np.uint64(0xFFFFFFFF))).astype(np.int64)
                fast += int((fused == s.pred_ids[row].cpu().numpy()).sum())
            n = s.steps_done
            out[arm].update(fast_branch_share=round(fast / (probe * B), 4), slow_branch_share=round(1 - fast / (probe * B), 4),
                            n_kept_mean=round(float(s.pred_n_kept[:n].float().mean()), 1), n_kept_max=int(s.pred_n_kept[:n].max()))
    a = out["a_sample"]
    res = dict(B=B, context=ctx, steps=steps, repeats=repeats, probe_steps=probe, decode="hipGraph", temperature=TEMPERATURE,
               a_spread_ms=round(a["max_ms"] - a["min_ms"], 4), **out)
    for arm in ("b_top_p", "c_top_k", "d_all", "e_unfused"):
        res[arm]["over_a_ms"] = round(out[arm]["ms_per_step"] - a["ms_per_step"], 4)
    res["not_slower_than_unfused"] = {arm: bool(out[arm]["ms_per_step"] <= out["e_unfused"]["ms_per_step"])
                                      for arm in ("b_top_p", "c_top_k", "d_all")}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--probe", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("truncated_sampling_bench needs a GPU")
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.config import UniMedVLConfig
    from unimedvl_amd.weights import random_getter
    cfg = UniMedVLConfig()
    model = Bagel(cfg, random_getter(cfg, "cuda", seed=1234), device="cuda", visual_gen=False, visual_und=True)
    res = dict(device=torch.cuda.get_device_name(0))
    with torch.no_grad():
        res["step"] = run(model.language_model, 8, 1060, args.steps, args.warmup, args.repeats, args.probe)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
