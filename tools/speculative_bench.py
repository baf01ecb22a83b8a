#!/usr/bin/env python
"""What a speculative greedy decode step costs and returns on the MI355X, at the full 14B dimensions with random weights, in one process.

A step of draft_len = k runs B * (k + 1) rows through the captured graph, so its time does not depend on how many drafts are accepted;
the tokens it emits do.  Random weights accept nothing through the prompt lookup, so acceptance is FORCED through predicted_ids (the
device tensor the captured step reads, rewritten between runs without a re-capture):
  0 %     random predictions: every step verifies k drafts, rejects them and emits one token;
  100 %   the arm's own greedy output as its prediction, found by iterating runs from the same start until the output reproduces the
          prediction (the rows of a window see other key splits than a one-token step, so a near-tie may flip between runs);
  ~50 %   that prediction with tokens corrupted at random, at the rate that accepts about half the drafts.
Arms: the plain session at B = 1 and B = 8 (the yardstick, same process, same weights), draft_len 3 and 7 at B = 1, 1 and 3 at B = 8;
context 1060 (zero keys / values: timing depends on lengths only).  Every timed run restarts from the same state - context 1060 - runs
`warmup` steps untimed and `steps` timed (graph replay), the arms of a batch size alternating, `repeats` times.  A speculative run ends
deeper in the context than the plain one (up to steps * (k + 1) tokens), which is counted against it.

Per arm: ms per step (median, min - max), tokens per step, ms per emitted token next to the plain arm's min - max, and the break-even:
the tokens per step at which ms per token equals the plain arm's median.

--sampled runs the sampled arms instead (speculative decode with sampling, SpeculativeDecodeSession(sampling=...)): B = 1 with k = 3 and
k = 7, B = 8 with k = 1, each with plain sampling (T = 1), with top_p = 0.9 and with log-probabilities.  A step's time does not depend on
what is accepted, so the predictions are the random ones (0 %).  Per arm, in the same process and alternating: the greedy speculative
step at the same (B, k), the plain per-row session at the same sampler, the plain scalar session; reported: the sampled step over the
greedy one, the rows session over the scalar one, what the sampled step costs beyond those two (the commit launch and the T - B extra
pick workgroups), and the break-even tokens per step against the plain per-row session.

    python tools/speculative_bench.py [--steps 64] [--warmup 8] [--repeats 3] [--sampled] [--out FILE]"""
import argparse
import gc
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

CTX = 1060
ARMS = {1: (3, 7), 8: (1, 3)}          # batch size -> draft lengths
SAMPLED_ARMS = {1: (3, 7), 8: (1,)}
SAMPLERS = {"sample": (dict(do_sample=True, temperature=1.0), False), "top_p": (dict(do_sample=True, temperature=1.0, top_p=0.9), False),
            "sample_logprobs": (dict(do_sample=True, temperature=1.0), True)}


def _timed(sess, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    sess.step(n)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


class Arm:
    """a session that can be put back to its first state"""

    def __init__(self, llm, B, k, total, sampling=None, logprobs=False, rows=False):
        """sampling (SamplingParams keywords): the sampled speculative session (k > 0), or with k = 0 the plain per-row session
        (rows=True) / the plain scalar session at the same sampler"""
        from unimedvl_amd.decode import DecodeSession
        from unimedvl_amd.kvcache import NaiveCache
        from unimedvl_amd.speculative import SpeculativeDecodeSession
        cfg, dev = llm.cfg, llm.device
        self.B, self.k = B, k
        self.room = total * (k + 1)
        cache = NaiveCache(cfg.layers)
        cache.ensure(B, CTX + self.room + k + 8, cfg.kv_heads, cfg.head_dim, dev)
        cache.lens = [CTX] * B
        start = torch.randint(1000, 100000, (B,), generator=torch.Generator().manual_seed(5))
        pos = torch.full((B,), CTX, dtype=torch.int64)
        extra = {}
        if sampling is not None:
            from unimedvl_amd.sampling import SamplingParams
            par = [SamplingParams(seed=77 + b, **sampling) for b in range(B)]
            extra = dict(sampling=par, logprobs=logprobs) if k else dict(row_sampling=par, logprobs=logprobs) if rows else \
                dict(sampling, seed=77, logprobs=logprobs)
        if k:
            g = torch.Generator().manual_seed(6 + k)
            self.garbage = torch.randint(1000, 100000, (B, self.room), generator=g).to(dev)
            self.sess = SpeculativeDecodeSession(llm, cache, start, pos, self.room, k, use_graph=True, predicted_ids=self.garbage.cpu(),
                                                 **extra)
        else:
            self.sess = DecodeSession(llm, cache, start, pos, self.room + 1, use_graph=True, **extra)
        self.first = [t.clone() for t in self.sess._state()]

    def reset(self, predicted=None):
        for t, v in zip(self.sess._state(), self.first):
            t.copy_(v)
        self.sess.steps_done = 0
        if predicted is not None:
            self.sess.predicted.copy_(predicted)
            self.sess._step_end(draft_only=True)       # the first step's drafts from the new prediction

    def own_output(self, steps, passes=24):
        """the prediction this arm reproduces over `steps` steps from the start: run, predict the output, run again"""
        pred = self.garbage.clone()
        for n in range(passes):
            self.reset(pred)
            self.sess.step(steps)
            out = self.sess.out_ids.clone()
            new = torch.where(torch.arange(self.room, device=out.device)[None, :] < self.sess.n_out[:, None].long(), out, self.garbage)
            if torch.equal(new, pred):           # (only once the run is covered: a garbage tail is rejected and replaced)
                return pred, n + 1
            pred = new
        return pred, passes

    def corrupted(self, pred, rate, seed):
        g = torch.Generator().manual_seed(seed)
        hit = (torch.rand(pred.shape, generator=g) < rate).to(pred.device)
        return torch.where(hit, (pred + 1) % 100000, pred)


def _half_rate(k):
    """the per-token corruption rate at which about half of k drafts are accepted: sum_j (1 - p)^j = k / 2"""
    lo, hi = 0.0, 1.0
    for _ in range(40):
        p = (lo + hi) / 2
        lo, hi = (p, hi) if sum((1 - p) ** j for j in range(1, k + 1)) > k / 2 else (lo, p)
    return (lo + hi) / 2


def batch_leg(llm, B, steps, warmup, repeats):
    total = warmup + steps
    plain = Arm(llm, B, 0, total)
    runs = [("plain", plain, None)]
    for k in ARMS[B]:
        arm = Arm(llm, B, k, total)
        own, passes = arm.own_output(total)
        for name, pred in (("0", arm.garbage), ("50", arm.corrupted(own, _half_rate(k), 40 + k)), ("100", own)):
            runs.append((f"k{k}_accept{name}", arm, pred))
        arm.passes = passes
    times = {name: [] for name, _, _ in runs}
    counts = {}
    for _ in range(repeats):
        for name, arm, pred in runs:
            arm.reset(pred)
            arm.sess.step(warmup)
            if arm.k:
                before = arm.sess.n_out.clone(), arm.sess.stats.clone()
            times[name].append(_timed(arm.sess, steps))
            if arm.k:
                emitted = (arm.sess.n_out - before[0]).float().mean().item()
                st = (arm.sess.stats - before[1]).sum(0).tolist()
                counts[name] = dict(tokens_per_step=round(emitted / steps, 3), drafted=st[1], accepted=st[2],
                                    acceptance=round(st[2] / max(st[1], 1), 3),
                                    context_end=CTX + int(arm.sess.n_out.max()))
    out = {}
    base = times["plain"]
    base_med = statistics.median(base)
    for name, arm, _ in runs:
        t = times[name]
        med = statistics.median(t)
        r = dict(rows=arm.B * (arm.k + 1), ms_per_step=round(med, 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4))
        if arm.k:
            tps = counts[name]["tokens_per_step"]
            r.update(counts[name], ms_per_token=round(med / tps, 4), break_even_tokens_per_step=round(med / base_med, 3),
                     speedup_over_plain=round(base_med / (med / tps), 3), fixed_point_passes=arm.passes)
        else:
            r.update(tokens_per_step=1.0, ms_per_token=round(med, 4), context_end=CTX + warmup + steps)
        out[name] = r
    res = dict(B=B, context=CTX, steps=steps, warmup=warmup, repeats=repeats, decode="hipGraph",
               plain_ms_per_token_min_max=[round(min(base), 4), round(max(base), 4)], arms=out)
    print(json.dumps(res), flush=True)
    return res


def sampled_leg(llm, B, steps, warmup, repeats):
    """the sampled arms of one batch size: per (k, sampler) four sessions timed alternating, `repeats` times"""
    total = warmup + steps
    out = {}
    for k in SAMPLED_ARMS[B]:
        greedy = Arm(llm, B, k, total)
        for name, (par, lp) in SAMPLERS.items():
            runs = [("sampled_spec", Arm(llm, B, k, total, par, lp)), ("greedy_spec", greedy), ("plain_rows", Arm(llm, B, 0, total, par, lp, rows=True)),
                    ("plain_scalar", Arm(llm, B, 0, total, par, lp))]
            times = {n: [] for n, _ in runs}
            for _ in range(repeats):
                for n, arm in runs:
                    arm.reset(arm.garbage if arm.k else None)
                    arm.sess.step(warmup)
                    times[n].append(_timed(arm.sess, steps))
            med = {n: statistics.median(t) for n, t in times.items()}
            r = {n: dict(ms_per_step=round(med[n], 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4)) for n, t in times.items()}
            r.update(rows=B * (k + 1), sampled_minus_greedy_spec_us=round(1e3 * (med["sampled_spec"] - med["greedy_spec"]), 2),
                     rows_minus_scalar_us=round(1e3 * (med["plain_rows"] - med["plain_scalar"]), 2),
                     beyond_both_us=round(1e3 * (med["sampled_spec"] - med["greedy_spec"] - (med["plain_rows"] - med["plain_scalar"])), 2),
                     break_even_tokens_per_step=round(med["sampled_spec"] / med["plain_rows"], 3))
            out[f"k{k}_{name}"] = r
            del runs
            gc.collect()
    res = dict(B=B, context=CTX, steps=steps, warmup=warmup, repeats=repeats, decode="hipGraph", arms=out)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--sampled", action="store_true", help="the sampled arms (B = 1: k = 3, 7; B = 8: k = 1) instead of the greedy ones")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("speculative_bench needs a GPU")
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.config import UniMedVLConfig
    from unimedvl_amd.weights import random_getter
    cfg = UniMedVLConfig()
    model = Bagel(cfg, random_getter(cfg, "cuda", seed=1234), device="cuda", visual_gen=False, visual_und=True)
    res = dict(device=torch.cuda.get_device_name(0), note="random weights: acceptance is forced through predicted_ids; the prompt "
               "lookup accepts nothing on random text, so real-text acceptance is not measured here")
    with torch.no_grad():
        for B in (int(v) for v in args.batches.split(",")):
            leg = sampled_leg if args.sampled else batch_leg
            res[f"B{B}"] = leg(model.language_model, B, args.steps, args.warmup, args.repeats)
            gc.collect()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
