#!/usr/bin/env python
"""What the logit penalties (repetition / presence / frequency penalty and logit bias in the decode step: one umv_logit_penalty_bf16
launch between the lm_head GEMM and the step end) cost on the MI355X, at the full 14B dimensions with random weights, in one process:
ms per decode step (graph replay), B = 8 at 1060 tokens of context (the headline run's), four arms on the same weights, alternated
REPEATS times, min - max per arm:

  a  penalties off (today's greedy step)
  b  greedy, repetition_penalty = 1.1                          (the visit list is the generated tokens: it grows by one per step)
  c  b plus a context set of 1024 distinct tokens per row      (the list starts 1024 long)
  d  do_sample, top_p = 0.9, logprobs, and b's penalty plus presence / frequency penalties and a two-entry logit bias

The added time per step of b, c and d over a is reported next to a's own min - max spread; the yardstick for "one latency-floor launch"
is the average of a small kernel (residual_rmsnorm) in a kernel trace of a decode run.

    python tools/penalty_bench.py [--steps 64] [--warmup 8] [--repeats 3] [--out profiles/penalty_decode_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

B, CONTEXT, CONTEXT_SET = 8, 1060, 1024
REP = dict(repetition_penalty=1.1)
ARMS = {
    "a_off": {},
    "b_repetition": dict(REP),
    "c_repetition_context": dict(REP, penalty_context_ids=True),
    "d_sample_top_p_logprobs": dict(REP, presence_penalty=0.5, frequency_penalty=0.25, logit_bias={11: 2.0, 12: float("-inf")},
                                    do_sample=True, temperature=1.0, seed=1234, top_p=0.9, logprobs=True),
}


def _timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(llm, steps, warmup, repeats):
    from unimedvl_amd.decode import DecodeSession
    from unimedvl_amd.kvcache import NaiveCache
    cfg, dev = llm.cfg, llm.device
    total = warmup + repeats * steps
    g = torch.Generator().manual_seed(5)
    context = [torch.randperm(cfg.vocab, generator=g)[:CONTEXT_SET].tolist() for _ in range(B)]
    sessions = {}
    for arm, kw in ARMS.items():
        kw = dict(kw)
        if kw.pop("penalty_context_ids", False):
            kw["penalty_context_ids"] = context
        cache = NaiveCache(cfg.layers)
        cache.ensure(B, CONTEXT + total + 8, cfg.kv_heads, cfg.head_dim, dev)
        cache.lens = [CONTEXT] * B           # a context of zero keys / values: timing depends on lengths only
        start = torch.randint(1000, 100000, (B,), generator=torch.Generator().manual_seed(5))
        sessions[arm] = DecodeSession(llm, cache, start, torch.full((B,), CONTEXT, dtype=torch.int64), total + 1, use_graph=True, **kw)
        sessions[arm].step(warmup)
    times = {a: [] for a in ARMS}
    for _ in range(repeats):
        for arm in ARMS:
            times[arm].append(_timed(lambda i, s=sessions[arm]: s.step(1), steps))
    out = {}
    for arm in ARMS:
        t, s = times[arm], sessions[arm]
        out[arm] = dict(ms_per_step=round(statistics.median(t), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4),
                        all_ms=[round(v, 4) for v in t])
        if s.pen is not None:
            out[arm]["list_length_at_end"] = [int(v) for v in s.pen_len.tolist()]
            out[arm]["distinct_generated"] = [int(v) - s.pen_static for v in s.pen_len.tolist()]
    a = out["a_off"]
    res = dict(B=B, context=CONTEXT, steps=steps, repeats=repeats, decode="hipGraph", a_spread_ms=round(a["max_ms"] - a["min_ms"], 4), **out)
    for arm in ARMS:
        if arm != "a_off":
            res[arm]["over_a_us"] = round((out[arm]["ms_per_step"] - a["ms_per_step"]) * 1000, 2)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("penalty_bench needs a GPU")
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.config import UniMedVLConfig
    from unimedvl_amd.weights import random_getter
    cfg = UniMedVLConfig()
    model = Bagel(cfg, random_getter(cfg, "cuda", seed=1234), device="cuda", visual_gen=False, visual_und=True)
    res = dict(device=torch.cuda.get_device_name(0))
    with torch.no_grad():
        res["step"] = run(model.language_model, args.steps, args.warmup, args.repeats)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
