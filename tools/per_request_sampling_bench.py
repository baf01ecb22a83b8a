#!/usr/bin/env python
"""What per-request sampling parameters (DecodeSession(row_sampling=...): the lm_head epilogue, the penalty kernel and
umv_decode_step_end_rows read one 48-byte table row per sample) cost on the MI355X, at the full 14B dimensions with random weights, in one
process: ms per decode step (graph replay), B = 8 at 1060 tokens of context (the headline run's).  Every pair is a scalar session and the
session whose table holds the same parameters in every row; a last arm mixes the four samplers over the rows.  The arms are alternated
REPEATS times, min - max per arm:

  greedy      scalar / rows          do_sample   scalar / rows (temperature 1)
  top_p       scalar / rows (0.9)    all         scalar / rows (top_p 0.9, log-probabilities, the three penalties)
  mixed       rows only: greedy, do_sample, top_p and all, two rows each (penalty buffers and log-probabilities on for the launch)

The time a rows arm adds over its scalar twin is reported next to the scalar arm's own min - max spread; the yardstick for "one
latency-floor launch" is the average of a small kernel (residual_rmsnorm, about 5 us) in a kernel trace of a decode run.

    python tools/per_request_sampling_bench.py [--steps 64] [--warmup 8] [--repeats 3] [--out profiles/per_request_sampling_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

B, CONTEXT, SEED = 8, 1060, 1234
PEN = dict(repetition_penalty=1.1, presence_penalty=0.5, frequency_penalty=0.25)
SAMPLERS = {
    "greedy": ({}, {}),
    "do_sample": (dict(do_sample=True, temperature=1.0), {}),
    "top_p": (dict(do_sample=True, temperature=1.0, top_p=0.9), {}),
    "all": (dict(do_sample=True, temperature=1.0, top_p=0.9, **PEN), dict(logprobs=True)),
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
    from unimedvl_amd.sampling import SamplingParams
    cfg, dev = llm.cfg, llm.device
    total = warmup + repeats * steps
    arms = {}
    for name, (smp, extra) in SAMPLERS.items():
        arms[name + "_scalar"] = dict(smp, **extra)
        arms[name + "_rows"] = dict(extra, row_sampling=[SamplingParams(**smp)] * B, row_streams=list(range(B)))
    arms["mixed_rows"] = dict(logprobs=True, row_sampling=[SamplingParams(**SAMPLERS[n][0]) for n in SAMPLERS for _ in range(B // len(SAMPLERS))])
    sessions = {}
    for arm, kw in arms.items():
        cache = NaiveCache(cfg.layers)
        cache.ensure(B, CONTEXT + total + 8, cfg.kv_heads, cfg.head_dim, dev)
        cache.lens = [CONTEXT] * B           # a context of zero keys / values: timing depends on lengths only
        start = torch.randint(1000, 100000, (B,), generator=torch.Generator().manual_seed(5))
        sessions[arm] = DecodeSession(llm, cache, start, torch.full((B,), CONTEXT, dtype=torch.int64), total + 1, use_graph=True, seed=SEED, **kw)
        sessions[arm].step(warmup)
    times = {a: [] for a in arms}
    for _ in range(repeats):
        for arm in arms:
            times[arm].append(_timed(lambda i, s=sessions[arm]: s.step(1), steps))
    out = {}
    for arm in arms:
        t = times[arm]
        out[arm] = dict(ms_per_step=round(statistics.median(t), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4),
                        all_ms=[round(v, 4) for v in t], step_end=sessions[arm].step_end)
    for name in SAMPLERS:
        sc, rw = out[name + "_scalar"], out[name + "_rows"]
        rw["over_scalar_us"] = round((rw["ms_per_step"] - sc["ms_per_step"]) * 1000, 2)
        rw["scalar_spread_us"] = round((sc["max_ms"] - sc["min_ms"]) * 1000, 2)
        same = torch.equal(sessions[name + "_scalar"].pred_ids, sessions[name + "_rows"].pred_ids)
        rw["same_tokens_as_scalar"] = bool(same)
    out["mixed_rows"]["over_all_scalar_us"] = round((out["mixed_rows"]["ms_per_step"] - out["all_scalar"]["ms_per_step"]) * 1000, 2)
    out["mixed_rows"]["over_greedy_scalar_us"] = round((out["mixed_rows"]["ms_per_step"] - out["greedy_scalar"]["ms_per_step"]) * 1000, 2)
    res = dict(B=B, context=CONTEXT, steps=steps, repeats=repeats, decode="hipGraph", table_bytes=48 * B, **out)
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
        raise SystemExit("per_request_sampling_bench needs a GPU")
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
