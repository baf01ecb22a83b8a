#!/usr/bin/env python
"""What each decode-step feature costs on the MI355X, at the full 14B dimensions with random weights, in one process: ms per decode
step (graph replay), B = 8 at 1060 tokens of context (the headline run's).  A suite is a set of arms (DecodeSession keywords) on the
same weights, alternated REPEATS times, median and min - max per arm; what an arm adds over its baseline arm is reported next to the
baseline's own min - max spread.  The yardstick for "one latency-floor launch" is the average of a small kernel (residual_rmsnorm,
about 5 us) in a kernel trace of a decode run: --trace-arm NAME runs that arm of the suite alone for --steps replays.

  penalties     a off | b greedy, repetition_penalty 1.1 (the visit list grows by one per step) | c b plus a context set of 1024 distinct
                tokens per row | d do_sample, top_p 0.9, logprobs, b's penalty plus presence / frequency penalties and a two-entry bias
  constraint    a off | b all rows on a 4-choice trie, greedy | c b with do_sample, top_p 0.9, logprobs (c0: that sampler, constraint
                off) | d one constrained row of 8 | e an allowed set of 10 000 tokens on all rows.  (A masked row costs the same in
                every state: every tile of it is rewritten.)
  ngram         a off | b greedy, no_repeat_ngram_size 3, generated history only | c b plus a 1024-token seeded context per row (the
                scan walks about 1.2 k int32 per row) | d do_sample, top_p 0.9, logprobs, repetition_penalty 1.1 and the same n = 3 (d0: that
                sampler and penalty, n-gram ban off)
  sequences     a off | b min_new_tokens 1000 alone (one single-token entry, active on every step) | c 64 bad words of 1 to 4 tokens |
                d a suppress list of 4096 tokens (every thread scans 16 entries and recomputes 16 tiles) | e beam search, 8 requests
                of 4 beams, with one 16-token bad word next to the 64: max_m = 16, every row walks 14 back-pointers (e0: the same
                search, stage off)
  logprobs      off | on, greedy; plus a `score` leg: one Bagel.score call (a 448 x 448 image, a 32-token question, four candidates of
                eight tokens) next to one Bagel.chat call with max_length = 9, each run twice - the warm time is the one to read
  top_logprobs  a greedy logprobs | b a + top 5 | c a + top 20 | s do_sample | d s + top_k 50: the yardstick - the selection runs the
                same cutoff once more over the row, so b - a and c - a are expected to be no more than d - s
  truncated     a do_sample | b top_p 0.9 | c top_k 50 | d top_k 50, top_p 0.9, min_p 0.05 | e the unfused sampler
                (UMV_DECODE_FUSED_ARGMAX=0 around the construction), the yardstick a truncated step has to beat.  Random weights give
                nearly flat logits: c drops the untruncated pick on almost every step (the slow branch), b keeps it with probability
                about 0.9.  The branch shares are counted on --probe further steps per arm, outside the timing: a step took the fast
                branch iff its token is the column of the largest lm_head key.
  beam          beam search decode (beam.BeamDecodeSession on a PagedCache, random weights and no end token, so every step reorders):
                b_beam_1x4 / c_beam_8x4 = 1 / 8 requests of 4 beams, each next to the plain greedy session with logprobs at the same
                row count (a_rows4 / a_rows32) - what the three launches that end a beam step add over the plain step end
  guidance      classifier-free guidance for text (guidance.GuidedDecodeSession): a_plain_8 plain, 8 rows | b_plain_16 plain, 16 rows (the
                same rows without the stage; logprobs on, as a guided session always runs with statistics) | c_guided_8x2 8 guided pairs,
                greedy, scale 3 | d_guided_8x2_sample_top_p_logprobs as c with do_sample, T = 0.7, top_p 0.9 and log-probabilities (d0: that
                sampler on 16 plain rows).  c - b is the stage's cost, b - a the price of the second row set
  per_request   greedy / do_sample / top_p / all (top_p, logprobs, the three penalties), each as a scalar session and as the session
                whose per-row table holds the same parameters in every row, and mixed_rows: the four samplers, two rows each
  all           every suite, the model loaded once

The JSON of a suite keeps the keys of the tool it replaces (profiles/*_bench.json).  Only the public session API is used, so the tool
runs against another checkout of the package on PYTHONPATH as well.

    python tools/decode_step_bench.py SUITE [--steps 64] [--warmup 8] [--repeats 3] [--probe 32] [--trace-arm ARM] [--context 1060] [--out FILE]"""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time
from collections import namedtuple

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # behind PYTHONPATH: a checkout named there wins
import numpy as np  # noqa: E402
import torch  # noqa: E402

B, CONTEXT, SEED, EOS = 8, 1060, 1234, 151645
# arms: {name: DecodeSession keywords, or a function of cfg that returns them}; over: (arm, baseline, key) - key ends in the unit;
# spread: (arm, key); head: further top-level keys; label: (key, {arm: what is stored under it}); hook(run, res): the extras
Suite = namedtuple("Suite", "arms over spread head label extra_steps hook", defaults=({}, None, 0, None))
Run = namedtuple("Run", "llm sessions out args")


def _timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


@contextlib.contextmanager
def _environ(env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _session(llm, kw, total):
    """rows (default B): the samples of the session; num_beams: a beam session of that many beams over `rows` requests on a paged cache"""
    from unimedvl_amd.decode import DecodeSession
    from unimedvl_amd.kvcache import NaiveCache
    cfg, dev = llm.cfg, llm.device
    kw = dict(kw(cfg) if callable(kw) else kw)
    n, beams, guided = kw.pop("rows", B), kw.pop("num_beams", 0), kw.pop("guidance_scale", None)
    start = torch.randint(1000, 100000, (n,), generator=torch.Generator().manual_seed(5))
    pos = torch.full((n,), CONTEXT, dtype=torch.int64)
    if beams:
        from unimedvl_amd.beam import BeamDecodeSession
        from unimedvl_amd.kvcache import PagedCache
        pages = (CONTEXT + total + 8) // 256 + 2
        cache = PagedCache(cfg.layers, pool_pages=n * pages * (1 + 2 * beams) + 1, max_context=pages * 256)
        cache.ensure_tokens([CONTEXT] * n, cfg.kv_heads, cfg.head_dim, dev)
        cache.lens = [CONTEXT] * n
        return BeamDecodeSession(llm, cache, start, pos, total + 2, beams, use_graph=True, **kw)
    cache = NaiveCache(cfg.layers)
    cache.ensure(n, CONTEXT + total + 8, cfg.kv_heads, cfg.head_dim, dev)
    cache.lens = [CONTEXT] * n           # a context of zero keys / values: timing depends on lengths only
    if guided is not None:               # n rows = n / 2 pairs: the conditional rows, then their partners
        from unimedvl_amd.guidance import GuidedDecodeSession
        return GuidedDecodeSession(llm, cache, start[:n // 2], pos[:n // 2], total + 1, guided, guidance_positions=pos[n // 2:],
                                   use_graph=True, **kw)
    with _environ(kw.pop("env", {})):
        return DecodeSession(llm, cache, start, pos, total + 1, use_graph=True, **kw)


def _diff(out, arm, base, key):
    d = out[arm]["ms_per_step"] - out[base]["ms_per_step"]
    return round(d * 1000, 2) if key.endswith("_us") else round(d, 4)


def run_suite(llm, suite, args):
    total = args.warmup + args.repeats * args.steps + (args.probe if suite.extra_steps else 0)
    sessions = {arm: _session(llm, kw, total) for arm, kw in suite.arms.items()}
    for s in sessions.values():
        s.step(args.warmup)
    times = {arm: [] for arm in sessions}
    for _ in range(args.repeats):
        for arm, s in sessions.items():
            times[arm].append(_timed(lambda i, s=s: s.step(1), args.steps))
    out = {}
    for arm, t in times.items():
        out[arm] = dict(ms_per_step=round(statistics.median(t), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4),
                        all_ms=[round(v, 4) for v in t])
        if suite.label:
            out[arm] = dict({suite.label[0]: suite.label[1][arm]}, **out[arm])
    res = dict(B=B, context=CONTEXT, steps=args.steps, repeats=args.repeats, decode="hipGraph", **suite.head)
    for arm, key in suite.spread:
        spread = out[arm]["max_ms"] - out[arm]["min_ms"]
        res[key] = round(spread * 1000, 2) if key.endswith("_us") else round(spread, 4)
    res.update(out)
    for arm, base, key in suite.over:
        res[arm][key] = _diff(out, arm, base, key)
    if suite.hook:
        suite.hook(Run(llm, sessions, out, args), res)
    print(json.dumps(res), flush=True)
    return res


# ---- penalties
def _context_set(cfg):
    g = torch.Generator().manual_seed(5)
    return dict(REP, penalty_context_ids=[torch.randperm(cfg.vocab, generator=g)[:1024].tolist() for _ in range(B)])


def _penalty_lists(run, res):
    for arm, s in run.sessions.items():
        if s.pen is not None:
            res[arm]["list_length_at_end"] = [int(v) for v in s.pen_len.tolist()]
            res[arm]["distinct_generated"] = [int(v) - s.pen_static for v in s.pen_len.tolist()]


REP = dict(repetition_penalty=1.1)
PENALTIES = Suite(
    arms={"a_off": {}, "b_repetition": dict(REP), "c_repetition_context": _context_set,
          "d_sample_top_p_logprobs": dict(REP, presence_penalty=0.5, frequency_penalty=0.25, logit_bias={11: 2.0, 12: float("-inf")},
                                          do_sample=True, temperature=1.0, seed=SEED, top_p=0.9, logprobs=True)},
    over=[(arm, "a_off", "over_a_us") for arm in ("b_repetition", "c_repetition_context", "d_sample_top_p_logprobs")],
    spread=[("a_off", "a_spread_ms")], hook=_penalty_lists)


# ---- constraint
def _automaton(kind, **kw):
    def build(cfg):
        from unimedvl_amd.constraints import TokenAutomaton
        if kind == "trie":      # four short answers, two of them sharing their first token
            return dict(kw, constraint=TokenAutomaton.from_choices([[9454], [2753], [21390, 387], [21390, 537]], EOS))
        ids = torch.randperm(cfg.vocab, generator=torch.Generator().manual_seed(7))[:10000].tolist()
        return dict(kw, constraint=TokenAutomaton.from_allowed_tokens(ids))
    return build


def _constraint_states(run, res):
    for arm, s in run.sessions.items():
        if s.con_state is not None:
            res[arm]["states_at_end"] = [int(v) for v in s.con_state.tolist()]
            res[arm]["masked_rows"] = sum(1 for v in s.con_state.tolist() if 0 <= int(v) < s.constraint.n_states)
            res[arm]["automaton"] = dict(states=s.constraint.n_states, edges=s.constraint.n_edges)


SAMPLED = dict(do_sample=True, temperature=1.0, seed=SEED, top_p=0.9, logprobs=True)
CONSTRAINT = Suite(
    arms={"a_off": {}, "b_trie_greedy": _automaton("trie"), "c_trie_sample_top_p_logprobs": _automaton("trie", **SAMPLED),
          "c0_sample_top_p_logprobs_off": dict(SAMPLED), "d_one_row_of_eight": _automaton("trie", constraint_states=[0] + [-1] * (B - 1)),
          "e_set_of_10000": _automaton("set")},
    over=[(arm, "a_off", "over_a_us") for arm in ("b_trie_greedy", "c_trie_sample_top_p_logprobs", "c0_sample_top_p_logprobs_off",
                                                  "d_one_row_of_eight", "e_set_of_10000")]
    + [("c_trie_sample_top_p_logprobs", "c0_sample_top_p_logprobs_off", "over_c0_us")],
    spread=[("a_off", "a_spread_ms"), ("c0_sample_top_p_logprobs_off", "c0_spread_ms")], hook=_constraint_states)


# ---- no-repeat n-grams
def _ngram_context(cfg):
    g = torch.Generator().manual_seed(5)
    return dict(NGRAM, ngram_context_ids=[torch.randint(1000, 100000, (1024,), generator=g).tolist() for _ in range(B)])


def _ngram_histories(run, res):
    for arm, s in run.sessions.items():
        if s.ng_hist is not None:
            res[arm]["history_length_at_end"] = [int(v) for v in s.ng_len.tolist()]
            res[arm]["history_room"] = int(s.ng_hist.shape[1])


NGRAM = dict(no_repeat_ngram_size=3)
NGRAM_SAMPLED = dict(REP, do_sample=True, temperature=1.0, seed=SEED, top_p=0.9, logprobs=True)
NGRAM_SUITE = Suite(
    arms={"a_off": {}, "b_ngram3": dict(NGRAM), "c_ngram3_context": _ngram_context,
          "d_sample_top_p_logprobs_penalty": dict(NGRAM, **NGRAM_SAMPLED), "d0_sample_top_p_logprobs_penalty_off": dict(NGRAM_SAMPLED)},
    over=[(arm, "a_off", "over_a_us") for arm in ("b_ngram3", "c_ngram3_context", "d_sample_top_p_logprobs_penalty",
                                                  "d0_sample_top_p_logprobs_penalty_off")]
    + [("d_sample_top_p_logprobs_penalty", "d0_sample_top_p_logprobs_penalty_off", "over_d0_us")],
    spread=[("a_off", "a_spread_ms"), ("d0_sample_top_p_logprobs_penalty_off", "d0_spread_ms")], hook=_ngram_histories)


# ---- banned sequences
def _bad_words(n, longest=4, extra=()):
    def build(cfg):
        g = torch.Generator().manual_seed(9)
        words = [torch.randint(1000, 100000, (1 + i % longest,), generator=g).tolist() for i in range(n)]
        return dict(bad_words_ids=words + [list(w) for w in extra])
    return build


def _suppress_list(cfg):
    return dict(suppress_tokens=torch.randperm(cfg.vocab, generator=torch.Generator().manual_seed(9))[:4096].tolist())


def _sequence_tables(run, res):
    for arm, s in run.sessions.items():
        if s.seq_table is not None:
            res[arm].update(entries=s.seq_table.S, table_tokens=s.seq_table.n_tok, max_m=s.seq_table.max_m)
            if s.seq_count is not None:
                res[arm]["count_at_end"] = [int(v) for v in s.seq_count.tolist()]


def _beamed(kw):
    return lambda cfg: dict(kw(cfg) if callable(kw) else kw, rows=8, num_beams=4)


SEQUENCES = Suite(
    arms={"a_off": {}, "b_min_new_tokens": dict(min_new_tokens=1000, end_token_id=EOS), "c_64_bad_words": _bad_words(64),
          "d_suppress_4096": _suppress_list, "e0_beam_8x4_off": _beamed({}),
          "e_beam_8x4_max_m16": _beamed(_bad_words(64, extra=[range(2000, 2016)]))},
    over=[(arm, "a_off", "over_a_us") for arm in ("b_min_new_tokens", "c_64_bad_words", "d_suppress_4096")]
    + [("e_beam_8x4_max_m16", "e0_beam_8x4_off", "over_e0_us")],
    spread=[("a_off", "a_spread_us"), ("e0_beam_8x4_off", "e0_spread_us")], hook=_sequence_tables)


# ---- logprobs
def _logprob_values(run, res):
    n = run.args.warmup + run.args.repeats * run.args.steps
    lp = run.sessions["on"].pred_logprobs[:n]
    res.update(same_token_ids=bool(torch.equal(run.sessions["off"].pred_ids[:n], run.sessions["on"].pred_ids[:n])),
               logprobs_finite=bool(torch.isfinite(lp).all()), logprob_mean=round(float(lp.mean()), 3),
               cost_ms=_diff(run.out, "on", "off", "cost_ms"), statistics_bytes_per_step=8 * B * ((run.llm.cfg.vocab + 15) // 16) * 2)


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


LOGPROBS = Suite(arms={"off": dict(logprobs=False), "on": dict(logprobs=True)}, over=[], spread=[("off", "off_spread_ms")],
                 hook=_logprob_values)


# ---- top_logprobs
def _ranked(run, res):
    yard = res["d_sample_top_k"]["over_s_ms"]
    res["no_more_than_truncated_step_end"] = {arm: bool(res[arm]["over_a_ms"] <= yard) for arm in ("b_top5", "c_top20")}
    # the sessions with the mode on really ranked the fed token: greedy, so every rank is 1 and the first alternative is the pick
    for arm in ("b_top5", "c_top20"):
        sn = run.sessions[arm]
        n = sn.steps_done
        assert bool((sn.pred_rank[:n] == 1).all()) and torch.equal(sn.pred_top_ids[:n, :, 0].long(), sn.pred_ids[:n]), arm


def _keyed(arms):
    """the arms of a sampled suite: every session gets the suite's temperature and seed; the label keeps the arm's own keywords"""
    return {arm: (lambda cfg, kw=kw: dict(kw, temperature=1.0, seed=SEED)) for arm, kw in arms.items()}


_TOP = {"a_logprobs": dict(logprobs=True), "b_top5": dict(logprobs=True, top_logprobs=5), "c_top20": dict(logprobs=True, top_logprobs=20),
        "s_sample": dict(do_sample=True), "d_sample_top_k": dict(do_sample=True, top_k=50)}
TOP_LOGPROBS = Suite(arms=_keyed(_TOP), over=[("b_top5", "a_logprobs", "over_a_ms"), ("c_top20", "a_logprobs", "over_a_ms"),
                                              ("d_sample_top_k", "s_sample", "over_s_ms")],
                     spread=[("a_logprobs", "a_spread_ms"), ("s_sample", "s_spread_ms")], head=dict(temperature=1.0), label=("session", _TOP),
                     hook=_ranked)


# ---- truncated sampling
def _branch_shares(run, res):
    probe = run.args.probe
    for arm, s in run.sessions.items():
        if s.truncated:
            fast = 0
            for _ in range(probe):
                row = s.steps_done
                s.step(1)
                key = s.amax_part.cpu().numpy().view(np.uint64).max(axis=1)          # the keys are unsigned
                fused = (np.uint64(0xFFFFFFFF) - (key & np.uint64(0xFFFFFFFF))).astype(np.int64)
                fast += int((fused == s.pred_ids[row].cpu().numpy()).sum())
            n = s.steps_done
            res[arm].update(fast_branch_share=round(fast / (probe * B), 4), slow_branch_share=round(1 - fast / (probe * B), 4),
                            n_kept_mean=round(float(s.pred_n_kept[:n].float().mean()), 1), n_kept_max=int(s.pred_n_kept[:n].max()))
    res["probe_steps"] = probe
    res["not_slower_than_unfused"] = {arm: bool(res[arm]["ms_per_step"] <= res["e_unfused"]["ms_per_step"])
                                      for arm in ("b_top_p", "c_top_k", "d_all")}


_FILTERS = {"a_sample": {}, "b_top_p": dict(top_p=0.9), "c_top_k": dict(top_k=50), "d_all": dict(top_k=50, top_p=0.9, min_p=0.05),
            "e_unfused": {}}
TRUNCATED = Suite(
    arms={arm: (lambda cfg, arm=arm, flt=flt: dict(flt, do_sample=True, temperature=1.0, seed=SEED,
                                                   env={"UMV_DECODE_FUSED_ARGMAX": "0"} if arm == "e_unfused" else {}))
          for arm, flt in _FILTERS.items()},
    over=[(arm, "a_sample", "over_a_ms") for arm in ("b_top_p", "c_top_k", "d_all", "e_unfused")], spread=[("a_sample", "a_spread_ms")],
    head=dict(temperature=1.0), label=("filters", _FILTERS), extra_steps=1, hook=_branch_shares)


# ---- per-request sampling
PEN = dict(repetition_penalty=1.1, presence_penalty=0.5, frequency_penalty=0.25)
SAMPLERS = {"greedy": ({}, {}), "do_sample": (dict(do_sample=True, temperature=1.0), {}),
            "top_p": (dict(do_sample=True, temperature=1.0, top_p=0.9), {}),
            "all": (dict(do_sample=True, temperature=1.0, top_p=0.9, **PEN), dict(logprobs=True))}


def _rows(samplers, **kw):
    def build(cfg):
        from unimedvl_amd.sampling import SamplingParams
        return dict(kw, seed=SEED, row_sampling=[SamplingParams(**SAMPLERS[n][0]) for n in samplers for _ in range(B // len(samplers))])
    return build


def _per_request_arms():
    arms = {}
    for name, (smp, extra) in SAMPLERS.items():
        arms[name + "_scalar"] = dict(smp, seed=SEED, **extra)
        arms[name + "_rows"] = _rows([name], row_streams=list(range(B)), **extra)
    arms["mixed_rows"] = _rows(list(SAMPLERS), logprobs=True)
    return arms


def _same_tokens(run, res):
    for arm, s in run.sessions.items():
        res[arm]["step_end"] = s.step_end
    for name in SAMPLERS:
        sc, rw = res[name + "_scalar"], res[name + "_rows"]
        rw["scalar_spread_us"] = round((sc["max_ms"] - sc["min_ms"]) * 1000, 2)
        rw["same_tokens_as_scalar"] = bool(torch.equal(run.sessions[name + "_scalar"].pred_ids, run.sessions[name + "_rows"].pred_ids))


PER_REQUEST = Suite(arms=_per_request_arms(), over=[(name + "_rows", name + "_scalar", "over_scalar_us") for name in SAMPLERS]
                    + [("mixed_rows", "all_scalar", "over_all_scalar_us"), ("mixed_rows", "greedy_scalar", "over_greedy_scalar_us")],
                    spread=[], head=dict(table_bytes=48 * B), hook=_same_tokens)

# ---- beam search decode
def _beam_reorders(run, res):
    for arm, s in run.sessions.items():
        if hasattr(s, "beam"):
            n, K = s.steps_done, s.K
            own = torch.arange(K, dtype=torch.int32, device=s.beam.beam_parent.device).repeat(s.requests)
            res[arm].update(rows=s.rows, nsplit=s.nsplit, done=s.done(),
                            rows_that_changed_parent=round(float((s.beam.beam_parent[:n] != own).float().mean()), 3))
        else:
            res[arm].update(rows=s.rows, nsplit=s.nsplit)


BEAM = Suite(arms={"a_rows4": dict(rows=4, logprobs=True), "b_beam_1x4": dict(rows=1, num_beams=4),
                   "a_rows32": dict(rows=32, logprobs=True), "c_beam_8x4": dict(rows=8, num_beams=4)},
             over=[("b_beam_1x4", "a_rows4", "over_plain_us"), ("c_beam_8x4", "a_rows32", "over_plain_us")],
             spread=[("a_rows4", "a_rows4_spread_us"), ("a_rows32", "a_rows32_spread_us")], hook=_beam_reorders)

# ---- classifier-free guidance for text
def _guidance_rows(run, res):
    for arm, s in run.sessions.items():
        res[arm].update(rows=s.rows, nsplit=s.nsplit, step_end=s.step_end)
        if getattr(s, "guid", None) is not None:
            res[arm].update(stage_launches=2 if s.guid["stats"] is None else 3, lse_finite=bool(torch.isfinite(s.lse).all()))
    res["stage_cost_us"] = _diff(run.out, "c_guided_8x2", "b_plain_16", "_us")
    res["second_row_set_us"] = _diff(run.out, "b_plain_16", "a_plain_8", "_us")
    res["sampled_stage_cost_us"] = _diff(run.out, "d_guided_8x2_sample_top_p_logprobs", "d0_plain_16_sample_top_p_logprobs", "_us")


GUIDED_SAMPLED = dict(do_sample=True, temperature=0.7, seed=SEED, top_p=0.9, logprobs=True)
GUIDANCE = Suite(
    arms={"a_plain_8": {}, "b_plain_16": dict(rows=16, logprobs=True), "c_guided_8x2": dict(rows=16, guidance_scale=3.0),
          "d_guided_8x2_sample_top_p_logprobs": dict(GUIDED_SAMPLED, rows=16, guidance_scale=3.0),
          "d0_plain_16_sample_top_p_logprobs": dict(GUIDED_SAMPLED, rows=16)},
    over=[("b_plain_16", "a_plain_8", "over_a_us"), ("c_guided_8x2", "b_plain_16", "over_b_us"),
          ("d_guided_8x2_sample_top_p_logprobs", "d0_plain_16_sample_top_p_logprobs", "over_d0_us")],
    spread=[("a_plain_8", "a_spread_us"), ("b_plain_16", "b_spread_us"), ("d0_plain_16_sample_top_p_logprobs", "d0_spread_us")],
    hook=_guidance_rows)

SUITES = {"penalties": PENALTIES, "constraint": CONSTRAINT, "ngram": NGRAM_SUITE, "sequences": SEQUENCES, "logprobs": LOGPROBS, "top_logprobs": TOP_LOGPROBS, "truncated": TRUNCATED,
          "per_request": PER_REQUEST, "beam": BEAM, "guidance": GUIDANCE}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("suite", choices=list(SUITES) + ["all"])
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--probe", type=int, default=32, help="truncated: further steps per arm on which the branch shares are counted")
    ap.add_argument("--legs", default="step,score", help="logprobs: which of its two legs to run")
    ap.add_argument("--trace-arm", default=None, help="run this arm of the suite alone, for a kernel trace of this tool")
    ap.add_argument("--context", type=int, default=CONTEXT, help="tokens of context per sample (beam: L mod 256 sets what a reorder copies)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    globals()["CONTEXT"] = args.context
    if not torch.cuda.is_available():
        raise SystemExit("decode_step_bench needs a GPU")
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.config import UniMedVLConfig
    from unimedvl_amd.weights import random_getter
    print(f"unimedvl_amd from {os.path.dirname(sys.modules['unimedvl_amd'].__file__)}", file=sys.stderr)
    cfg = UniMedVLConfig()
    model = Bagel(cfg, random_getter(cfg, "cuda", seed=1234), device="cuda", visual_gen=False, visual_und=True)
    res = dict(device=torch.cuda.get_device_name(0))
    with torch.no_grad():
        if args.trace_arm:
            if args.suite == "all" or args.trace_arm not in SUITES[args.suite].arms:
                raise SystemExit("--trace-arm names an arm of the one suite given")
            s = _session(model.language_model, SUITES[args.suite].arms[args.trace_arm], args.warmup + args.steps)
            s.step(args.warmup + args.steps)
            torch.cuda.synchronize()
            return
        for name in (SUITES if args.suite == "all" else [args.suite]):
            one = res.setdefault(name, {}) if args.suite == "all" else res
            if name != "logprobs" or "step" in args.legs.split(","):
                one["step"] = run_suite(model.language_model, SUITES[name], args)
            if name == "logprobs" and "score" in args.legs.split(","):
                one["score"] = score_leg(model, cfg)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
