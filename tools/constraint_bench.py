#!/usr/bin/env python
"""What constrained decoding (a token automaton masks the logits inside the decode step: umv_logit_constrain_bf16 between the lm_head
GEMM and the step end, umv_constraint_advance behind it) costs on the MI355X, at the full 14B dimensions with random weights, in one
process: ms per decode step (graph replay), B = 8 at 1060 tokens of context (the headline run's), five arms on the same weights,
alternated REPEATS times, min - max per arm:

  a  constraint off (today's greedy step)
  b  all 8 rows on a 4-choice trie, greedy
  c  b with do_sample, top_p = 0.9 and log-probabilities     (c0: the same sampler with the constraint off, c's own control)
  d 1 constrained row of 8 (the others carry state -1)
  e  an allowed set of 10 000 tokens on all rows

(The rows of b, c and d reach the trie's final state after a few steps and stay on its end-token self-loop: a masked row costs the
same in every state - every tile of it is rewritten.)  The added time per step over a is reported next to a's own min - max spread;
the yardstick for "one latency-floor launch" is the average of a small kernel (residual_rmsnorm) in a kernel trace of a decode run:
--trace-arm NAME runs that arm alone for --steps replays, for a kernel trace of this tool.

    python tools/constraint_bench.py [--steps 64] [--warmup 8] [--repeats 3] [--out profiles/constraint_decode_bench.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

B, CONTEXT, EOS = 8, 1060, 151645
TRIE = [[9454], [2753], [21390, 387], [21390, 537]]        # four short answers, two of them sharing their first token
SAMPLED = dict(do_sample=True, temperature=1.0, seed=1234, top_p=0.9, logprobs=True)
ARMS = {
    "a_off": {},
    "b_trie_greedy": dict(constraint="trie"),
    "c_trie_sample_top_p_logprobs": dict(constraint="trie", **SAMPLED),
    "c0_sample_top_p_logprobs_off": dict(SAMPLED),
    "d_one_row_of_eight": dict(constraint="trie", constraint_states=[0] + [-1] * (B - 1)),
    "e_set_of_10000": dict(constraint="set"),
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


def _session(llm, arm, total):
    from unimedvl_amd.constraints import TokenAutomaton
    from unimedvl_amd.decode import DecodeSession
    from unimedvl_amd.kvcache import NaiveCache
    cfg, dev = llm.cfg, llm.device
    kw = dict(ARMS[arm])
    if kw.get("constraint") == "trie":
        kw["constraint"] = TokenAutomaton.from_choices(TRIE, EOS)
    elif kw.get("constraint") == "set":
        kw["constraint"] = TokenAutomaton.from_allowed_tokens(torch.randperm(cfg.vocab, generator=torch.Generator().manual_seed(7))[:10000].tolist())
    cache = NaiveCache(cfg.layers)
    cache.ensure(B, CONTEXT + total + 8, cfg.kv_heads, cfg.head_dim, dev)
    cache.lens = [CONTEXT] * B           # a context of zero keys / values: timing depends on lengths only
    start = torch.randint(1000, 100000, (B,), generator=torch.Generator().manual_seed(5))
    return DecodeSession(llm, cache, start, torch.full((B,), CONTEXT, dtype=torch.int64), total + 1, use_graph=True, **kw)


def run(llm, steps, warmup, repeats):
    total = warmup + repeats * steps
    sessions = {}
    for arm in ARMS:
        sessions[arm] = _session(llm, arm, total)
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
        if s.con_state is not None:
            out[arm]["states_at_end"] = [int(v) for v in s.con_state.tolist()]
            out[arm]["masked_rows"] = sum(1 for v in s.con_state.tolist() if 0 <= int(v) < s.constraint.n_states)
            out[arm]["automaton"] = dict(states=s.constraint.n_states, edges=s.constraint.n_edges)
    a = out["a_off"]
    res = dict(B=B, context=CONTEXT, steps=steps, repeats=repeats, decode="hipGraph", a_spread_ms=round(a["max_ms"] - a["min_ms"], 4), **out)
    for arm in ARMS:
        if arm != "a_off":
            res[arm]["over_a_us"] = round((out[arm]["ms_per_step"] - a["ms_per_step"]) * 1000, 2)
    c, c0 = res["c_trie_sample_top_p_logprobs"], res["c0_sample_top_p_logprobs_off"]
    c["over_c0_us"] = round((c["ms_per_step"] - c0["ms_per_step"]) * 1000, 2)
    res["c0_spread_ms"] = round(c0["max_ms"] - c0["min_ms"], 4)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trace-arm", default=None, choices=list(ARMS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("constraint_bench needs a GPU")
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.config import UniMedVLConfig
    from unimedvl_amd.weights import random_getter
    cfg = UniMedVLConfig()
    model = Bagel(cfg, random_getter(cfg, "cuda", seed=1234), device="cuda", visual_gen=False, visual_und=True)
    res = dict(device=torch.cuda.get_device_name(0))
    with torch.no_grad():
        if args.trace_arm:
            s = _session(model.language_model, args.trace_arm, args.warmup + args.steps)
            s.step(args.warmup + args.steps)
            torch.cuda.synchronize()
            return
        res["step"] = run(model.language_model, args.steps, args.warmup, args.repeats)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
