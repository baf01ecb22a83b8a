"""Speculative greedy decode: every step verifies draft_len drafted tokens per sample next to the sample's own next token, so one pass
over the weights can emit up to draft_len + 1 tokens - and never a token plain greedy decoding would not have emitted.

The drafts need no second model: they are read off the request's own text (prompt lookup: the most recent earlier occurrence of the
last few tokens, and what followed it) or off a continuation the caller predicts (predicted_ids).  A step is DecodeSession's step over
B * (draft_len + 1) rows - umv_qkv_post appends all of them, umv_attn_varlen masks them causally (max_q = draft_len + 1), the lm_head
epilogue leaves every row's argmax keys - and umv_decode_step_end_speculative ends it on the device: verify, emit, advance the sample's
length by what was accepted (the rejected rows' K/V stays above the length and is overwritten by the next step), append to the
history, draft again.  So the whole step still replays as one graph with no host round trip.

Greedy: a verified token is the argmax of the logits its row computed.  Sampled (sampling=): a request's noise is keyed by its own
(seed, stream, draw), so row j of a sample draws with the key of the token it would emit, its pick is the plain per-row session's pick
after the same prefix, and a draft is accepted exactly when it equals that pick - no rejection-sampling arithmetic.  Either way the
rows of a step see the same keys a plain step would, but the attention's key split depends on the segment's length, so a logit may
differ from the plain step's in the last bit."""
import inspect
import os

import torch

from . import ops
from .decode import DecodeSession
from .sampling import per_sample


def _token_lists(value, B, what):
    """per sample a list of ints from None, a [B, n] tensor or a sequence of B sequences"""
    if value is None:
        return [[] for _ in range(B)]
    rows = value.tolist() if hasattr(value, "tolist") else [list(r.tolist() if hasattr(r, "tolist") else r) for r in value]
    if len(rows) != B or any(not isinstance(r, list) for r in rows):
        raise ValueError(f"{what} must hold one token list per sample ({B})")
    return [[int(t) for t in r] for r in rows]


# DecodeSession's keywords that pick a sampler, log, force, penalise or constrain - every parameter behind nsplit, with its default:
# all of them must be at their neutral value here.  (temperature and seed mean nothing without do_sample and are ignored.)
_IGNORED = ("temperature", "seed")
_NEUTRAL = {name: p.default for name, p in inspect.signature(DecodeSession.__init__).parameters.items()}
_NEUTRAL = {name: _NEUTRAL[name] for name in list(_NEUTRAL)[list(_NEUTRAL).index("nsplit") + 1:] if name not in _IGNORED}


def _neutral(name, v):
    if name not in _NEUTRAL:
        raise TypeError(f"SpeculativeDecodeSession got an unexpected keyword argument {name!r}")
    want = _NEUTRAL[name]
    if want is None:
        return v is None or (name == "logit_bias" and not v)
    return isinstance(v, (bool, int, float)) and v == want


class SpeculativeDecodeSession(DecodeSession):
    def __init__(self, llm, cache, start_tokens, positions, max_length, draft_len, use_graph=True, nsplit=None, *, draft_ngram=(2, 4),
                 draft_context_ids=None, predicted_ids=None, sampling=None, sampling_streams=None, **plain):
        """max_length: tokens to emit per sample at the most (out_ids [B, max_length] int64, n_out [B] int32: how many of a row are
        valid).  limit ([B] int32, device, starts at max_length): a sample stops emitting at out_ids[b][limit[b]] - the host may
        rewrite it between replays.  stats ([B, 3] int32): steps, drafts verified, drafts accepted.  draft_ngram = (min, max): the
        suffix lengths the prompt lookup tries, longest first.  draft_context_ids: per sample the tokens that precede the start token
        (the prompt; negative entries are separators nothing matches) - the history the lookup searches, which the emitted tokens
        extend.  predicted_ids: per sample a predicted continuation (what out_ids is expected to hold); a sample that has one drafts
        from it instead of the lookup.
        sampling (one sampling.SamplingParams, or a list of B): sampled speculative decode - every request verifies its drafts against
        its own seeded draw (include/unimedvl_hip.h, speculative decode with sampling), so out_ids is what
        DecodeSession(row_sampling=sampling, row_streams=sampling_streams, seed=seed) emits, token for token (up to the last bit of a
        logit: the attention's key split depends on the segment length).  The table has B * (draft_len + 1) entries; the step ends with
        umv_decode_pick_rows and umv_decode_step_end_speculative_rows.  sampling_streams: the `stream` word of every sample's key
        (default: the sample index, DecodeSession's default); seed: the seed of the params that carry none.  Greedy entries
        (SamplingParams()) are legal and may be mixed with sampled ones.  logprobs=True (with sampling): out_logprobs (fp32
        [B, max_length]) holds every emitted token's log-probability next to out_ids.  Penalised params, logit_bias, forced_ids,
        top_logprobs, constraint and no_repeat_ngram_size (the keyword, or a size in a SamplingParams) raise ValueError.
        Without sampling, any sampler, log-probability, forced-token, penalty, per-row, constraint or n-gram keyword raises ValueError."""
        k = int(draft_len)
        B = len(cache.lens)
        params, logprobs, seed = None, False, 0
        if sampling is not None:
            params = per_sample(sampling, B)
            if any(p.penalised for p in params):
                raise ValueError("sampled speculative decode takes no penalties (a penalised SamplingParams)")
            if any(p.no_repeat_ngram_size for p in params):
                raise ValueError("speculative decode takes no no_repeat_ngram_size (a SamplingParams with a size)")
            logprobs, seed = bool(plain.pop("logprobs", False)), int(plain.get("seed", 0))
        elif sampling_streams is not None:
            raise ValueError("sampling_streams goes with sampling")
        mode = "speculative decode is greedy only and" if params is None else "sampled speculative decode"
        on = [name for name, v in plain.items() if name not in _IGNORED and not _neutral(name, v)]
        if on:
            raise ValueError(("speculative decode is greedy only: no sampling, logprobs / forced_ids, penalties / logit_bias, constraint or "
                              "row_sampling" if params is None else
                              "sampled speculative decode takes its samplers from sampling=: no scalar sampler keywords, forced_ids, "
                              "penalties / logit_bias, top_logprobs, constraint or row_sampling") + f" (got {on})")
        if k < 1:
            raise ValueError(f"speculative decode needs draft_len >= 1 (got {draft_len})")
        if B * (k + 1) > 64:
            raise ValueError(f"{mode} rides on the fused step end: B * (draft_len + 1) = {B} x {k + 1} rows exceed its 64")
        if os.environ.get("UMV_DECODE_FUSED_ARGMAX", "1") in ("0", ""):
            raise ValueError(f"{mode} rides on the fused step end: UMV_DECODE_FUSED_ARGMAX=0 excludes it")
        lo, hi = (int(v) for v in draft_ngram)
        if not 1 <= lo <= hi:
            raise ValueError(f"draft_ngram = (min, max) with 1 <= min <= max, got {draft_ngram!r}")
        self.draft_len, self.draft_ngram = k, (lo, hi)
        with ops.device_scope(llm.device):
            self._init(llm, cache, start_tokens, positions, max_length, use_graph=False, nsplit=nsplit, seed=seed, logprobs=logprobs,
                       row_sampling=params, row_streams=sampling_streams)
            self._init_drafts(_token_lists(draft_context_ids, B, "draft_context_ids"), predicted_ids)
            if use_graph:
                self._capture()

    def _init_drafts(self, context, predicted):
        dev, B, k, V = self.dev, self.B, self.draft_len, self.cfg.vocab
        i32 = dict(dtype=torch.int32, device=dev)
        room = max(self.max_length, 1)
        self.out_ids = torch.zeros((B, room), dtype=torch.int64, device=dev)
        self.n_out = torch.zeros((B,), **i32)
        self.limit = torch.full((B,), self.max_length, **i32)
        self.n_draft = torch.zeros((B,), **i32)
        self.stats = torch.zeros((B, 3), **i32)
        self.out_logprobs = torch.zeros((B, room), dtype=torch.float32, device=dev) if self.logprobs else None
        # the history: the context, the start token, then what is emitted
        start = self.ids[::k + 1].tolist()
        rows = [c + [t] for c, t in zip(context, start)]
        hist = torch.zeros((B, max(len(r) for r in rows) + room), dtype=torch.int32)
        for b, r in enumerate(rows):
            if r and (max(r) >= 1 << 31 or min(r) < -(1 << 31)):
                raise ValueError("draft_context_ids holds a token that is no int32")
            hist[b, :len(r)] = torch.tensor(r, dtype=torch.int32)
        self.hist = hist.to(dev)
        self.hist_len = torch.tensor([len(r) for r in rows], dtype=torch.int32).to(dev)
        self.predicted = self.pred_len = None
        if predicted is not None:
            pred = _token_lists(predicted, B, "predicted_ids")
            t = torch.full((B, max(max(len(p) for p in pred), 1)), -1, dtype=torch.int64)
            for b, p in enumerate(pred):
                t[b, :len(p)] = torch.tensor(p, dtype=torch.int64)
            self.predicted = t.to(dev)
            self.pred_len = torch.tensor([len(p) for p in pred], dtype=torch.int32).to(dev)
        self._step_end(draft_only=True)          # the first step's drafts

    def _step_end(self, draft_only=False):
        spec = (self.ids, self.out_ids, self.n_out, self.limit, self.n_draft, self.hist, self.hist_len, self.stats, self.draft_len,
                self.cfg.vocab)
        kw = dict(ngram=self.draft_ngram, predicted=self.predicted, pred_len=self.pred_len, draft_only=draft_only)
        if self.row_table is None:
            ops.decode_step_end_speculative(self.tok_slot, self.tok_pos, self.kv_len, self.amax_part, *spec, **kw)
            return
        # sampled: every row's own pick (T workgroups sweep their rows in parallel), then the commit per sample - which also moves the
        # rows' draw counters to the sample's new token count and logs the emitted tokens' log-probabilities
        if not draft_only:
            ops.decode_pick_rows(self.amax_part, self.logits, self.row_table, self.row_picks, lse_partial=self.lse_part,
                                 logprob=self.row_logprob, cut_y=self.row_cut_y, n_kept=self.row_n_kept)
        ops.decode_step_end_speculative_rows(self.tok_slot, self.tok_pos, self.kv_len, self.row_picks, self.row_table, *spec, **kw,
                                             row_logprob=self.row_logprob, out_logprobs=self.out_logprobs)

    def _state(self):
        return super()._state() + (self.out_ids, self.n_out, self.n_draft, self.hist, self.hist_len, self.stats)

    def set_slot(self, *a, **kw):
        raise ValueError("a speculative session serves one set of requests from start to end (no set_slot / rewind_outputs)")

    rewind_outputs = set_slot

    def commit(self, rows=None):
        """Make the cache's host-side lengths lens0 + rows: the start token and the first rows - 1 emitted tokens are in the cache
        (default: what every sample has emitted)."""
        rows = int(self.n_out.min()) if rows is None else int(rows)
        self.cache.lens = [n + rows for n in self.lens0]
