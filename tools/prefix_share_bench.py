#!/usr/bin/env python
"""What sharing prefixes saves in the paged batcher on the MI355X: ContinuousBatcher(paged=True) with share_prefixes off against on, at
the full 14B dimensions with random weights, in one process.

Workload: 8 slots, 32 requests = 4 distinct 448 x 448 images x 8 questions of 32 tokens (question-major: the first admission group holds
every image twice), max_new_tokens 16, check_every 8.  A new batcher per run, so no entry outlives a run.  Arms, alternating, `repeats`
times after one untimed run each (graph capture, code objects, allocator):
  same_images   sharing off / on: the on arm should save about 28 image admissions
  distinct      32 distinct images, off / on: nothing hits - the price of hashing and bookkeeping, to be read against the off arm's spread
  admission     one image-chunk admission alone and one question-only admission alone (host packing + the pass, one request, slot 0)
Times are host clocks around calls that end in a device synchronise.  Reported: median, min - max in ms, requests per second, and the
measured saving against 28 x the measured image admission.

    python tools/prefix_share_bench.py [--repeats 3] [--out profiles/prefix_share_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

SLOTS, IMAGES, QUESTIONS, QUESTION_TOKENS, NEW_TOKENS, CHECK_EVERY = 8, 4, 8, 32, 16, 8


class IdTok:
    """a prompt is the index of a fixed list of token ids"""

    def __init__(self, table):
        self.table = table

    def encode(self, s):
        return list(self.table[int(s)])

    def decode(self, ids):
        return "<|im_start|>" + " ".join(str(int(v)) for v in ids[1:]) + "<|im_end|>"


def _stat(ts):
    return dict(median_ms=round(statistics.median(ts), 2), min_ms=round(min(ts), 2), max_ms=round(max(ts), 2))


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prefix_share_bench needs a GPU")
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.config import UniMedVLConfig
    from unimedvl_amd.serving import ContinuousBatcher
    from unimedvl_amd.weights import random_getter
    cfg = UniMedVLConfig()
    model = Bagel(cfg, random_getter(cfg, "cuda", seed=1234), device="cuda", visual_gen=False, visual_und=True)
    ntid = dict(bos_token_id=cfg.vocab - 4, eos_token_id=cfg.vocab - 3, start_of_image=cfg.vocab - 2, end_of_image=cfg.vocab - 1)
    g = torch.Generator().manual_seed(7)
    n_req = IMAGES * QUESTIONS
    images = [torch.randn(3, 448, 448, generator=g).clamp(-1, 1) for _ in range(n_req)]
    tok = IdTok([torch.randint(1000, 100000, (QUESTION_TOKENS,), generator=g).tolist() for _ in range(n_req)])

    def batcher(share):
        return ContinuousBatcher(model, tok, ntid, lambda x: x, slots=SLOTS, max_context=2048, max_new_tokens=NEW_TOKENS,
                                 check_every=CHECK_EVERY, paged=True, share_prefixes=share)

    def serve(share, distinct):
        srv = batcher(share)
        for i in range(n_req):                                   # question-major: request i asks question i about image i % 4
            srv.submit([images[i if distinct else i % IMAGES]], str(i))
        out = srv.run()
        return [out[r] for r in sorted(out)], dict(srv.stats)

    res = dict(device=torch.cuda.get_device_name(0), slots=SLOTS, requests=n_req, question_tokens=QUESTION_TOKENS, max_new_tokens=NEW_TOKENS,
               check_every=CHECK_EVERY, repeats=args.repeats, arms={})
    for name, distinct in (("same_images", False), ("distinct", True)):
        first = {share: serve(share, distinct) for share in (False, True)}          # untimed; and the answers agree
        times = {False: [], True: []}
        for _ in range(args.repeats):
            for share in (False, True):
                times[share].append(_wall(lambda: serve(share, distinct))[0])
        arm = dict(answers_equal=first[False][0] == first[True][0], stats_on=first[True][1])
        for share, key in ((False, "off"), (True, "on")):
            arm[key] = dict(_stat(times[share]), requests_per_s=round(n_req / (statistics.median(times[share]) / 1e3), 2))
        arm["saving_ms"] = round(arm["off"]["median_ms"] - arm["on"]["median_ms"], 2)
        res["arms"][name] = arm
        print(json.dumps({name: arm}), flush=True)

    # one admission alone, chunk by chunk, as serving._prefill_many runs it for a single request in slot 0
    srv = batcher(False)
    full = lambda v: torch.cat([v.cpu(), torch.zeros(SLOTS - 1, dtype=v.dtype)])   # noqa: E731

    def image_chunk(i):
        gi, kvl, rope = model.prepare_vit_images([0], [0], [images[i]], lambda x: x, ntid)
        gi["packed_seqlens"] = full(gi["packed_seqlens"])
        gi["key_values_lens"] = gi["packed_key_value_indexes"] = gi["packed_indexes"] = None
        model.forward_cache_update_vit(srv.cache, **gi)
        return kvl, rope

    def question_chunk(i, kvl, rope):
        gi, kvl, rope = model.prepare_prompts(kvl, rope, [str(i)], tok, ntid)
        gi["text_token_lens"] = full(gi["text_token_lens"])
        gi["key_values_lens"] = gi["packed_key_value_indexes"] = gi["packed_text_indexes"] = None
        model.forward_cache_update_text(srv.cache, **gi)

    t_img, t_txt = [], []
    for i in range(args.repeats + 1):
        srv.cache.release(0)
        t, (kvl, rope) = _wall(lambda: image_chunk(i))
        t_img.append(t)
        t_txt.append(_wall(lambda: question_chunk(i, kvl, rope))[0])
    adm = dict(image_chunk=_stat(t_img[1:]), question_chunk=_stat(t_txt[1:]), context_tokens_after_image=kvl[0])
    expected = 28 * adm["image_chunk"]["median_ms"]
    adm["expected_saving_ms"] = round(expected, 2)
    adm["measured_over_expected"] = round(res["arms"]["same_images"]["saving_ms"] / expected, 3)
    res["admission"] = adm
    print(json.dumps({"admission": adm}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
