#!/usr/bin/env python
"""What scoring given candidates costs on the MI355X: the forced decode session (Bagel.score) against the prefill-time scorer
(Bagel.score_prefill), at the full 14B dimensions with random weights, in one process.

Context: one 448 x 448 image and a 32-token question, prefilled by every call (all arms pay it).  Cases: 4 candidates of 64 tokens and
8 of 256 (the end token appended: 260 and 2056 rows).  Arms, alternating, `repeats` times after one untimed call each (graph capture,
code objects, allocator):
  1  score                       one forced decode step per token
  2  score_prefill(fused=False)  one prefill pass; lm_head stores logits chunk by chunk, token_logprob reads them back
  3  score_prefill               one prefill pass; lm_head leaves tile statistics and one logit per row
  4  the lm_head stage alone (Qwen2MoT.token_logprobs on the case's row count), fused against unfused, `inner` calls per timing
Times are host clocks around calls that end in a device synchronise (the results come back as host lists); arm 4 uses device events.
Reported per arm: median, min - max in ms; for arm 4 also the workspace bytes of either form and the peak of torch's allocator over
the call.

    python tools/score_bench.py [--repeats 3] [--inner 10] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

CASES = {"4x64": (4, 64), "8x256": (8, 256)}
QUESTION_TOKENS = 32


class IdTok:
    """the question is a fixed list of token ids; candidates are given as ids and never pass through here"""

    def __init__(self, ids):
        self.ids = ids

    def encode(self, s):
        return list(self.ids)


def _stat(ts):
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3))


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_bench needs a GPU")
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.config import UniMedVLConfig
    from unimedvl_amd.weights import random_getter
    cfg = UniMedVLConfig()
    model = Bagel(cfg, random_getter(cfg, "cuda", seed=1234), device="cuda", visual_gen=False, visual_und=True)
    lm = model.language_model
    ntid = dict(bos_token_id=cfg.vocab - 4, eos_token_id=cfg.vocab - 3, start_of_image=cfg.vocab - 2, end_of_image=cfg.vocab - 1)
    g = torch.Generator().manual_seed(7)
    img = torch.randn(3, 448, 448, generator=g).clamp(-1, 1)
    tok = IdTok(torch.randint(1000, 100000, (QUESTION_TOKENS,), generator=g).tolist())
    res = dict(device=torch.cuda.get_device_name(0), context="one 448 x 448 image + a 32-token question, prefilled inside every call",
               repeats=args.repeats, inner=args.inner, cases={})
    for name, (n, m) in CASES.items():
        cands = torch.randint(1000, 100000, (n, m), generator=g).tolist()
        arms = {"1_score": lambda: model.score(tok, ntid, lambda x: x, [img], "q", cands),
                "2_score_prefill_unfused": lambda: model.score_prefill(tok, ntid, lambda x: x, [img], "q", cands, fused=False),
                "3_score_prefill": lambda: model.score_prefill(tok, ntid, lambda x: x, [img], "q", cands)}
        out = {k: fn() for k, fn in arms.items()}                    # untimed first calls; and the three agree
        times = {k: [] for k in arms}
        for _ in range(args.repeats):
            for k, fn in arms.items():
                times[k].append(_wall(fn))
        flat = {k: torch.tensor([v for r in o for v in r["token_logprobs"]], dtype=torch.float64) for k, o in out.items()}
        case = dict(candidates=n, tokens=m, rows=n * (m + 1), arms={k: _stat(t) for k, t in times.items()},
                    largest_abs_difference=dict(prefill_vs_score=float((flat["3_score_prefill"] - flat["1_score"]).abs().max()),
                                                fused_vs_unfused=float((flat["3_score_prefill"] - flat["2_score_prefill_unfused"]).abs().max())))
        # arm 4: the lm_head stage alone on this case's row count
        T = n * (m + 1)
        hidden = torch.randn(T, cfg.hidden, generator=g).to(torch.bfloat16).cuda()
        ids = torch.randint(0, cfg.vocab, (T,), generator=g).cuda()
        stage, info = {True: [], False: []}, {}
        for fused in (True, False):                                   # untimed first calls
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            lm.token_logprobs(hidden, ids, fused=fused)
            torch.cuda.synchronize()
            info[fused] = dict(lm.last_token_logprobs, allocator_peak_bytes=torch.cuda.max_memory_allocated() - base)
        for _ in range(args.repeats):
            for fused in (True, False):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.inner):
                    lm.token_logprobs(hidden, ids, fused=fused)
                e1.record()
                torch.cuda.synchronize()
                stage[fused].append(e0.elapsed_time(e1) / args.inner)
        case["4_lm_head_stage"] = dict(rows=T, fused=dict(_stat(stage[True]), **info[True]), unfused=dict(_stat(stage[False]), **info[False]))
        res["cases"][name] = case
        print(json.dumps({name: case}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
