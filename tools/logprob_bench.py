#!/usr/bin/env python
"""What token log-probabilities cost on the MI355X, at the full 14B dimensions with random weights, in one process:

  step   ms per greedy decode step (graph replay), B = 8 at 1060 tokens of context (the headline run's): DecodeSession(logprobs=False)
         against logprobs=True on the same weights, alternated REPEATS times; min - max per arm.  Expected from bytes: the statistics
         are 8 B x 9504 bytes written and read once (0.6 MB at B = 8) plus one bf16 read per sample - about a microsecond.
  score  one Bagel.score call - one 448 x 448 image, a 32-token question, four candidates of eight tokens - next to one Bagel.chat
         call with max_length = 9 on the same image and question: what scoring costs relative to generating.  Each is run twice; the
         second (warm) time is the one to read.

    python tools/logprob_bench.py [--steps 64] [--warmup 8] [--repeats 3] [--legs step,score] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

ARMS = ("off", "on")


def _timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def step_leg(llm, B, ctx, steps, warmup, repeats):
    from unimedvl_amd.decode import DecodeSession
    from unimedvl_amd.kvcache import NaiveCache
    cfg, dev = llm.cfg, llm.device
    sessions = {}
    total = warmup + repeats * steps
    for arm in ARMS:
        cache = NaiveCache(cfg.layers)
        cache.ensure(B, ctx + total + 8, cfg.kv_heads, cfg.head_dim, dev)
        cache.lens = [ctx] * B           # a context of zero keys / values: timing depends on lengths only
        start = torch.randint(1000, 100000, (B,), generator=torch.Generator().manual_seed(5))
        sessions[arm] = DecodeSession(llm, cache, start, torch.full((B,), ctx, dtype=torch.int64), total + 1, use_graph=True,
                                      logprobs=arm == "on")
        sessions[arm].step(warmup)
    times = {a: [] for a in ARMS}
    for _ in range(repeats):
        for arm in ARMS:
            times[arm].append(_timed(lambda i, s=sessions[arm]: s.step(1), steps))
    n = warmup + repeats * steps
    same = torch.equal(sessions["off"].pred_ids[:n], sessions["on"].pred_ids[:n])
    lp = sessions["on"].pred_logprobs[:n]
    out = {}
    for arm in ARMS:
        t = times[arm]
        out[arm] = dict(ms_per_step=round(statistics.median(t), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4),
                        all_ms=[round(v, 4) for v in t])
    res = dict(B=B, context=ctx, steps=steps, repeats=repeats, decode="hipGraph", same_token_ids=bool(same),
               logprobs_finite=bool(torch.isfinite(lp).all()), logprob_mean=round(float(lp.mean()), 3),
               cost_ms=round(out["on"]["ms_per_step"] - out["off"]["ms_per_step"], 4),
               off_spread_ms=round(out["off"]["max_ms"] - out["off"]["min_ms"], 4),
               statistics_bytes_per_step=8 * B * ((cfg.vocab + 15) // 16) * 2, **out)
    print(json.dumps(res), flush=True)
    return res


def score_leg(model, cfg):
    class Tok:
        def __init__(self, ids):
            self.ids = ids

        def encode(self, s):
            return self.ids

        def decode(self, ids):
            return "<|im_start|>" + " ".join(str(int(i)) for i in ids[1:])
    ntid = dict(bos_token_id=cfg.vocab - 4, eos_token_id=cfg.vocab - 3, start_of_image=cfg.vocab - 2, end_of_image=cfg.vocab - 1)
    g = torch.Generator().manual_seed(11)
    img = torch.rand(3, 448, 448, generator=g) * 2 - 1
    tok = Tok(torch.randint(1000, 100000, (32,), generator=g).tolist())
    cands = [torch.randint(1000, 100000, (8,), generator=g).tolist() for _ in range(4)]
    res = {"image": "448x448", "question_tokens": 32, "candidates": 4, "candidate_tokens": 8}
    for name, fn in (("chat_max_length_9", lambda: model.chat(tok, ntid, lambda x: x, [img], "q", max_length=9)),
                     ("score_4x8", lambda: model.score(tok, ntid, lambda x: x, [img], "q", cands, append_eos=False))):
        ts = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(round((time.perf_counter() - t0) * 1e3, 2))
        res[name + "_ms"] = dict(first=ts[0], warm=ts[1])
        if name.startswith("score"):
            res["score_logprobs"] = [round(r["logprob"], 3) for r in out]
    res["score_over_chat"] = round(res["score_4x8_ms"]["warm"] / res["chat_max_length_9_ms"]["warm"], 3)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--legs", default="step,score")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("logprob_bench needs a GPU")
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.config import UniMedVLConfig
    from unimedvl_amd.weights import random_getter
    cfg = UniMedVLConfig()
    model = Bagel(cfg, random_getter(cfg, "cuda", seed=1234), device="cuda", visual_gen=False, visual_und=True)
    res = dict(device=torch.cuda.get_device_name(0))
    legs = args.legs.split(",")
    with torch.no_grad():
        if "step" in legs:
            res["step"] = step_leg(model.language_model, 8, 1060, args.steps, args.warmup, args.repeats)
        if "score" in legs:
            res["score"] = score_leg(model, cfg)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
