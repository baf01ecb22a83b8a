#!/usr/bin/env python
"""What the top-n alternatives (DecodeSession(top_logprobs=n): one umv_decode_top_logprobs launch behind the step end) cost on the
MI355X, at the full 14B dimensions with random weights, in one process: ms per decode step (graph replay), B = 8 at 1060 tokens of
context (the headline run's), five arms on the same weights, alternated REPEATS times, min - max per arm:

  a  greedy, logprobs=True (umv_decode_step_end_logprob)
  b  a + top_logprobs=5          c  a + top_logprobs=20
  s  do_sample as today (the lm_head sampling epilogue + umv_decode_step_end_argmax)
  d  s + top_k = 50 (umv_decode_step_end_truncated): the yardstick - the selection runs the same cutoff once more over the row, so
     b - a and c - a are expected to be no more than d - s

Random weights give nearly flat logits: the cutoff class of the n-th value holds few columns, as on real logits.

    python tools/top_logprobs_bench.py [--steps 64] [--warmup 8] [--repeats 3] [--out profiles/top_logprobs_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

ARMS = {"a_logprobs": dict(logprobs=True), "b_top5": dict(logprobs=True, top_logprobs=5), "c_top20": dict(logprobs=True, top_logprobs=20),
        "s_sample": dict(do_sample=True), "d_sample_top_k": dict(do_sample=True, top_k=50)}
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


def run(llm, B, ctx, steps, warmup, repeats):
    from unimedvl_amd.decode import DecodeSession
    from unimedvl_amd.kvcache import NaiveCache
    cfg, dev = llm.cfg, llm.device
    total = warmup + repeats * steps
    sessions = {}
    for arm, kw in ARMS.items():
        cache = NaiveCache(cfg.layers)
        cache.ensure(B, ctx + total + 8, cfg.kv_heads, cfg.head_dim, dev)
        cache.lens = [ctx] * B           # a context of zero keys / values: timing depends on lengths only
        start = torch.randint(1000, 100000, (B,), generator=torch.Generator().manual_seed(5))
        sessions[arm] = DecodeSession(llm, cache, start, torch.full((B,), ctx, dtype=torch.int64), total + 1, use_graph=True,
                                      temperature=TEMPERATURE, seed=SEED, **kw)
        sessions[arm].step(warmup)
    times = {a: [] for a in ARMS}
    for _ in range(repeats):
        for arm in ARMS:
            times[arm].append(_timed(lambda i, s=sessions[arm]: s.step(1), steps))
    out = {}
    for arm, kw in ARMS.items():
        t = times[arm]
        out[arm] = dict(session=kw, ms_per_step=round(statistics.median(t), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4),
                        all_ms=[round(v, 4) for v in t])
    a, s = out["a_logprobs"], out["s_sample"]
    for arm in ("b_top5", "c_top20"):
        out[arm]["over_a_ms"] = round(out[arm]["ms_per_step"] - a["ms_per_step"], 4)
    yard = round(out["d_sample_top_k"]["ms_per_step"] - s["ms_per_step"], 4)
    out["d_sample_top_k"]["over_s_ms"] = yard
    res = dict(B=B, context=ctx, steps=steps, repeats=repeats, decode="hipGraph", temperature=TEMPERATURE,
               a_spread_ms=round(a["max_ms"] - a["min_ms"], 4), s_spread_ms=round(s["max_ms"] - s["min_ms"], 4), **out)
    res["no_more_than_truncated_step_end"] = {arm: bool(out[arm]["over_a_ms"] <= yard) for arm in ("b_top5", "c_top20")}
    # the sessions with the mode on really ranked the fed token: greedy, so every rank is 1 and the first alternative is the pick
    for arm in ("b_top5", "c_top20"):
        sn = sessions[arm]
        n = sn.steps_done
        assert bool((sn.pred_rank[:n] == 1).all()) and torch.equal(sn.pred_top_ids[:n, :, 0].long(), sn.pred_ids[:n]), arm
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
        raise SystemExit("top_logprobs_bench needs a GPU")
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.config import UniMedVLConfig
    from unimedvl_amd.weights import random_getter
    cfg = UniMedVLConfig()
    model = Bagel(cfg, random_getter(cfg, "cuda", seed=1234), device="cuda", visual_gen=False, visual_und=True)
    res = dict(device=torch.cuda.get_device_name(0))
    with torch.no_grad():
        res["step"] = run(model.language_model, 8, 1060, args.steps, args.warmup, args.repeats)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
