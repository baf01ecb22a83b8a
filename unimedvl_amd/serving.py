"""Continuous (in-flight) batching for VQA decode - SURVEY.md section 8f rank 4 ("serving-grade decode").

The reference decodes one request at a time and stops a whole batch when SAMPLE 0 emits EOS
(codes/modeling/unimedvl/bagel.py:1262-1314).  Here B cache segments ("slots") decode together in ONE captured HIP
graph (decode.DecodeSession); every `check_every` steps the host looks at the generated ids, retires the slots that
produced <|im_end|> (or hit their token budget) and prefills the next queued request straight into the freed slot:

  * the KV cache is one slab per layer with a per-slot capacity reserved up front (kvcache.NaiveCache.reserve), so a new
    request is a prefill on a ONE-SEGMENT VIEW of that slab (NaiveCache.view_segments) - no copy, no re-allocation, the other
    slots' keys are untouched;
  * a request whose context does not fit that reservation GROWS the slabs (growable=True, the default: the reference's
    NaiveCache grows without bound, qwen2_navit.py:585-600): between two decode rounds the cache doubles
    (NaiveCache.ensure copies the committed keys), the decode session is re-captured on the new slabs and every active
    slot continues from its next token - answers are unchanged (tests/test_serving_gpu.py).  growable=False keeps the
    old contract: such a request is refused (ValueError) and nothing is re-allocated;
  * the graph reads each slot's next token / cache length / rope position from device memory
    (DecodeSession.set_slot), so re-pointing a slot needs no re-capture;
  * samples are independent rows of every kernel: a request's tokens are the same whichever slot and neighbours it gets
    (tests/test_serving_gpu.py checks this against one-request-at-a-time greedy decoding).
"""
import dataclasses
from collections import deque
from dataclasses import dataclass, field
from typing import Any, Deque, Dict, List, Optional

import torch

from . import ops

from .decode import DecodeSession
from .kvcache import NaiveCache, PagedCache
from .prefix import PrefixTable, adopt_point, chunk_keys, plan_group
from .sampling import SamplingParams, derive_seed, from_keywords


@dataclass
class _Request:
    rid: int
    images: List[Any]
    prompt: str
    max_new_tokens: int
    tokens: List[int] = field(default_factory=list)
    logprobs: List[float] = field(default_factory=list)
    top: List[Any] = field(default_factory=list)        # top_logprobs: per emitted token its n (id, logprob) pairs
    ranks: List[int] = field(default_factory=list)      # ... and the token's own rank
    prompt_ids: Optional[List[int]] = None      # penalize_prompt: the prompt's tokens, the repetition penalty's context set
    sampling: Optional[SamplingParams] = None   # per_request_sampling: the request's own parameters (None = the batcher's)
    constraint: Optional[str] = None            # the name of the automaton (ContinuousBatcher(constraints=)) the request decodes under
    image_keys: Optional[List[Any]] = None      # share_prefixes: the caller's own keys for the images (None = digests of the inputs)
    min_new_tokens: Optional[int] = None        # the request's own minimum before the end token may come (None = the batcher's)


class ContinuousBatcher:
    def __init__(self, model, tokenizer, new_token_ids, image_transform, slots: int = 8, max_context: int = 2048,
                 max_new_tokens: int = 256, check_every: int = 16, do_sample: bool = False, temperature: float = 1.0,
                 use_graph: bool = True, growable: bool = True, context_limit: Optional[int] = None, paged: bool = False,
                 pool_pages: Optional[int] = None, logprobs: bool = False, *, repetition_penalty: float = 1.0,
                 presence_penalty: float = 0.0, frequency_penalty: float = 0.0, logit_bias=None, penalize_prompt: bool = False,
                 per_request_sampling: bool = False, seed: Optional[int] = None, top_logprobs: int = 0, constraints=None,
                 no_repeat_ngram_size: int = 0, no_repeat_ngram_prompt: bool = False, share_prefixes: bool = False,
                 prefix_cache_pages: Optional[int] = None, bad_words_ids=None, bad_words=None, suppress_tokens=None,
                 begin_suppress_tokens=None, min_new_tokens: int = 0, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0):
        """max_context: the context (prompt + images) the slots are RESERVED for; with growable=True longer requests enlarge
        the cache (up to context_limit tokens of context when given), with growable=False they are refused.
        paged=True: block-table KV (kvcache.PagedCache) instead of slabs - the slots draw 256-token pages from ONE pool of `pool_pages`
        pages per layer (default: what max_context + max_new_tokens needs for every slot, plus as much again), a request of any length
        up to context_limit (default 32 768) is admitted without re-allocating or re-capturing anything, and a finished request returns
        its pages.  Same answers as the slab cache (tests/test_paged_kv_gpu.py).
        logprobs=True: self.logprobs[rid] holds one float per emitted token of the request - the token's log-probability as
        DecodeSession(logprobs=True) records it - cut at EOS or the budget exactly as the tokens are.  Needs slots <= 64.
        top_logprobs=n (1..20, batcher-wide: the buffer size is captured; implies logprobs): self.top_logprobs[rid] holds per emitted
        token a list of its n most likely alternatives as (id, logprob) pairs, most likely first, and self.ranks[rid] the token's own
        1-based rank (DecodeSession(top_logprobs=n)), both cut exactly as the tokens are.  Works with per_request_sampling.
        top_k / top_p / min_p: truncated sampling (DecodeSession), batcher-wide like temperature; they need do_sample and slots <= 64.
        repetition_penalty / presence_penalty / frequency_penalty / logit_bias: the logit penalties (DecodeSession), batcher-wide like
        temperature; a slot's history starts over when a request is admitted to it and lives across the rounds of that request.
        penalize_prompt=True: a request's prompt token ids (the text between the bos / eos wrapper, which is NOT part of the set: a
        penalised end token would only make answers longer) are its context set for the repetition penalty.  The session reserves
        room for the longest prompt admitted so far (a power of two, at least 32 distinct tokens) - the penalty kernel walks that
        reservation every step - and the step is re-captured, histories carried over, when a longer prompt arrives.
        per_request_sampling=True: every request decodes with its OWN sampling.SamplingParams (submit(..., sampling=)) inside the one
        captured step (DecodeSession(row_sampling=...)); the sampler keywords above become the default of the requests that give
        none, logit_bias stays batcher-wide.  A request's sampling key is (its seed, stream 0, its own draw counter from 0): the seed
        is SamplingParams.seed or, without one, derived on the host from `seed` (None: one draw from the model's generator at the
        first run()) and the request id - so a request's tokens and log-probabilities depend on neither its slot, its neighbours,
        the admission order nor check_every, and no noise repeats from round to round.  Needs slots <= 64.  False: nothing changes -
        one sampler for all, keyed by slot and round-local step.
        constraints ({name: constraints.TokenAutomaton}): constrained decoding (DecodeSession(constraint=)) - submit(..., constraint=name)
        decodes that request under the named automaton from its state 0; a request without one is free and decodes as it does in a
        batcher without constraints.  The automata are merged ONCE, here (TokenAutomaton.union), so the device tables have a captured
        size and never move; admission writes the request's start state into its slot's state word, and a re-captured session takes
        the live slots' words over as it takes the penalty histories over.  An automaton per request, compiled at submit, is not
        offered: the tables would have to grow under a captured step.
        no_repeat_ngram_size (0 = off): no request repeats an n-gram of that size (DecodeSession; HF's NoRepeatNGramLogitsProcessor) -
        batcher-wide like temperature, and under per_request_sampling the default of the requests whose SamplingParams give none.  A
        slot's history starts over when a request is admitted to it and lives across the rounds of that request; the session reserves
        it as the penalty context room is reserved - for the longest prompt and token budget admitted so far - and the step is
        re-captured, histories carried over, when a longer one arrives.  no_repeat_ngram_prompt=True seeds a request's history with
        its prompt's token ids (the text between the bos / eos wrapper, exactly the list penalize_prompt uses), so that an n-gram of
        the prompt is not repeated either; the default counts generated tokens only.  (HF's generate counts the prompt.)
        share_prefixes=True (needs paged=True): requests with the same images share their KV pages.  A request's chunks are its images
        in order, then its prompt; after every chunk a request computes, its context is retained under the tuple of the chunk keys so
        far (prefix.chunk_keys: digests of the raw images - or submit(image_keys=) - and the prompt's packed token ids), and a later
        request whose chain starts with a retained one adopts it - the full pages by reference count, the partially filled page as a
        private copy (PagedCache.adopt_prefix) - and prefills only the rest; inside one admission group the first request with a new
        key computes the chunk and the others copy from its slot right after the pass.  Sharing at chunk boundaries is exact: tokens
        and log-probabilities are those of the batcher with the option off (tests/test_prefix_share_gpu.py) wherever a pass stays on
        the same side of the 64-row GEMM split as in that run - always, for images of real size.  The entries live across
        rounds and run() calls, hold at most prefix_cache_pages distinct pages (default: a quarter of the pool), least recently used
        out first, and give way whenever a call that takes pages would not fit the free list - so sharing never fails a run that the
        same pool serves without it.  drop_prefixes() empties the table.  stats: prefix_hits (adoptions), prefix_tokens_reused,
        vit_images (images that went through the ViT), prefix_evictions.  False: nothing changes.
        bad_words_ids / suppress_tokens / begin_suppress_tokens (HF's keywords; DecodeSession, include/unimedvl_hip.h banned sequences):
        ONE batcher-wide table of token sequences no request may emit, tokens it never emits and tokens it does not emit first - the
        table has a captured size, so a table per request is not offered.  bad_words (strings): each is encoded bare and with a
        leading space (a word at the start of a text and inside a sentence are different tokens) and both join bad_words_ids
        (ops.encode_bad_words).  min_new_tokens: the end token is banned for a request's first that many tokens - the batcher-wide
        default, submit(..., min_new_tokens=) gives a request its own (one word per slot on the device, no re-capture: run() builds
        its step for what has been submitted).  A slot's count and last tokens start over
        when a request is admitted to it and live across its rounds.  The history is the fed tokens: a bad word that begins in the
        prompt is not seen.  All off: nothing changes."""
        if (share_prefixes or prefix_cache_pages is not None) and not paged:
            raise ValueError("share_prefixes / prefix_cache_pages need paged=True: prefixes are shared page by page")
        if prefix_cache_pages is not None and (not share_prefixes or int(prefix_cache_pages) < 0):
            raise ValueError(f"prefix_cache_pages (got {prefix_cache_pages!r}) is a page count >= 0 and goes with share_prefixes=True")
        self.constraint, self.constraint_start = None, {}
        if constraints:
            from .constraints import TokenAutomaton
            self.constraint, self.constraint_start = TokenAutomaton.union(dict(constraints))
        # the batcher-wide sampler keywords as one SamplingParams: checked here (a filter needs do_sample), and the default of the
        # requests that give none under per_request_sampling
        self.default_sampling = from_keywords(do_sample, temperature, top_k=top_k, top_p=top_p, min_p=min_p,
                                              repetition_penalty=repetition_penalty, presence_penalty=presence_penalty,
                                              frequency_penalty=frequency_penalty, no_repeat_ngram_size=no_repeat_ngram_size)
        self.ngram_prompt = bool(no_repeat_ngram_prompt)
        # banned sequences: the batcher-wide table (DecodeSession's keywords) and the default minimum; _min_on: does any request (or the
        # default) hold the end token back?  Then the session carries the end-token entry and one minimum per slot
        eos_id = int(new_token_ids["eos_token_id"])
        words, suppress, begin, self.min_new, _ = ops.check_sequences(
            list(bad_words_ids or []) + ops.encode_bad_words(tokenizer, bad_words), suppress_tokens, begin_suppress_tokens, min_new_tokens,
            eos_id, vocab=model.cfg.vocab)
        if isinstance(self.min_new, list):
            raise ValueError("min_new_tokens is one integer, the batcher-wide default: submit(..., min_new_tokens=) gives a request its own")
        self.banned = dict(bad_words_ids=words, suppress_tokens=suppress, begin_suppress_tokens=begin) if words or suppress or begin else {}
        self._min_on = self.min_new > 0
        self._ng_on = self.default_sampling.no_repeat_ngram_size > 0      # does any request (or the default) carry a size?
        self._ng_room = self._ng_hist = 0                                  # context / fed tokens per slot the decode session reserves
        self.top_k, self.top_p, self.min_p = self.default_sampling.top_k, self.default_sampling.top_p, self.default_sampling.min_p
        self.model, self.tokenizer, self.new_token_ids, self.image_transform = model, tokenizer, new_token_ids, image_transform
        self.device = model.device
        self.penalties = dict(zip(("repetition_penalty", "presence_penalty", "frequency_penalty", "logit_bias"),
                                  ops.check_penalties(repetition_penalty, presence_penalty, frequency_penalty, logit_bias,
                                                      vocab=model.cfg.vocab)))
        self.penalize_prompt = bool(penalize_prompt)
        self.per_request = bool(per_request_sampling)
        self.seed = None if seed is None else int(seed)
        if self.per_request:
            if int(slots) > 64:
                raise ValueError(f"per_request_sampling rides on the fused step end: at most 64 slots (got {slots})")
            # the session reserves the penalty buffers as soon as any request (or the default) is penalised
            self._row_pen = self.default_sampling.penalised
        elif seed is not None:
            raise ValueError("seed goes with per_request_sampling (the batcher-wide sampler draws its key from the model's generator)")
        self._pen_room = 0                              # distinct context tokens per slot the decode session reserves
        self.slots, self.check_every = int(slots), int(check_every)
        self.max_context, self.default_new = int(max_context), int(max_new_tokens)
        self.do_sample, self.temperature, self.use_graph = do_sample, temperature, use_graph
        self.growable, self.context_limit = bool(growable), context_limit
        self._grew = False
        cfg = model.cfg
        self.paged = bool(paged)
        per_slot = self.max_context + self.default_new + self.check_every + 8
        if self.paged:
            pages = 2 * self.slots * ((per_slot + ops.KV_PAGE - 1) // ops.KV_PAGE) + 1 if pool_pages is None else int(pool_pages)
            self.cache = PagedCache(cfg.layers, pool_pages=pages, max_context=(context_limit or 32768) + self.default_new + self.check_every + 8)
        else:
            self.cache = NaiveCache(cfg.layers)
        self.cache.reserve(self.slots, per_slot, cfg.kv_heads, cfg.head_dim, model.device)
        self.queue: Deque[_Request] = deque()
        self.results: Dict[int, str] = {}
        self.n_top = ops.check_top_logprobs(top_logprobs, cfg.vocab)
        self.want_logprobs = bool(logprobs) or self.n_top > 0
        self.logprobs: Dict[int, List[float]] = {}
        self.top_logprobs: Dict[int, List[Any]] = {}
        self.ranks: Dict[int, List[int]] = {}
        self._next_id = 0
        self.stats = {"decode_steps": 0, "prefills": 0, "tokens": 0, "cache_grows": 0}
        self.prefixes = None                # share_prefixes: the retained prefixes (prefix.PrefixTable)
        if share_prefixes:
            self.stats.update({"prefix_hits": 0, "prefix_tokens_reused": 0, "vit_images": 0})
            bound = (self.cache.pool_pages - 1) // 4 if prefix_cache_pages is None else int(prefix_cache_pages)
            self.prefixes = PrefixTable(self.cache, bound, self.stats)

    # ------------------------------------------------------------------ API
    def submit(self, images, prompt: str, max_new_tokens: Optional[int] = None, sampling: Optional[SamplingParams] = None,
               constraint: Optional[str] = None, image_keys=None, min_new_tokens: Optional[int] = None) -> int:
        """images: one image / a list of images (PIL or [3,H,W] tensors, as the transform accepts) or None.
        image_keys (share_prefixes=True; ignored without): one hashable key per image, used instead of a digest of the image's bytes
        (a study / series id, say).  They are trusted: equal keys must mean equal images.
        sampling (per_request_sampling=True only): the request's own SamplingParams; None = the batcher's defaults.
        constraint: the name of one of the batcher's automata (ContinuousBatcher(constraints=)); None = free text.
        min_new_tokens: the end token is banned for the request's first that many tokens; None = the batcher's default."""
        if min_new_tokens is not None:
            min_new_tokens = ops.check_sequences(min_new_tokens=min_new_tokens, end_token_id=0)[3]
            if isinstance(min_new_tokens, list):
                raise ValueError("submit(min_new_tokens=...) takes one integer")
            self._min_on = self._min_on or min_new_tokens > 0
        if constraint is not None and constraint not in self.constraint_start:
            raise ValueError(f"submit(constraint={constraint!r}): the batcher holds {sorted(self.constraint_start) or 'no automata'}")
        if sampling is not None:
            if not self.per_request:
                raise ValueError("submit(sampling=...) needs ContinuousBatcher(per_request_sampling=True)")
            if not isinstance(sampling, SamplingParams):
                raise ValueError(f"sampling must be a SamplingParams, got {type(sampling).__name__}")
            self._row_pen = self._row_pen or sampling.penalised
            self._ng_on = self._ng_on or sampling.no_repeat_ngram_size > 0
        imgs = [] if images is None else (list(images) if isinstance(images, (list, tuple)) else [images])
        if image_keys is not None:
            image_keys = list(image_keys) if isinstance(image_keys, (list, tuple)) else [image_keys]
            if len(image_keys) != len(imgs):
                raise ValueError(f"submit(image_keys=...): {len(image_keys)} keys for {len(imgs)} images")
            for key in image_keys:
                hash(key)
        budget = self.default_new if max_new_tokens is None else int(max_new_tokens)
        if budget > self.default_new and not self.growable:
            raise ValueError(f"max_new_tokens {budget} exceeds the batcher's reserve of {self.default_new}")
        rid = self._next_id
        self._next_id += 1
        self.queue.append(_Request(rid, imgs, prompt, budget, sampling=sampling, constraint=constraint, image_keys=image_keys,
                                   min_new_tokens=min_new_tokens))
        return rid

    def drop_prefixes(self):
        """share_prefixes: forget every retained prefix (its pages go back to the pool unless a live request still shares them)"""
        if self.prefixes is not None:
            self.prefixes.clear()

    @torch.no_grad()
    @ops.on_device
    def run(self) -> Dict[int, str]:
        """Serve everything that has been submitted; returns {request id: answer}."""
        m, cache, B = self.model, self.cache, self.slots
        bos, eos = self.new_token_ids["bos_token_id"], self.new_token_ids["eos_token_id"]
        active: List[Optional[_Request]] = [None] * B
        state = [(bos, 0, 0)] * B                       # (next token, kv_len, rope position) per slot
        for b in range(B):
            self._free_slot(b)
        first = []
        for b in range(B):
            if self.queue:
                active[b] = self.queue.popleft()
                first.append(b)
        for b, st in zip(first, self._prefill_many(first, [active[b] for b in first])):
            state[b] = st
        seed = m._sampling_seed() if self.do_sample and not self.per_request else 0
        if self.per_request and self.seed is None:
            self.seed = m._sampling_seed()

        def params_of(b):         # the parameters slot b decodes with: its request's (seeded by the request id), the default when idle
            req = active[b]
            if req is None:
                return self.default_sampling
            p = req.sampling or self.default_sampling
            return p if p.seed is not None else dataclasses.replace(p, seed=derive_seed(self.seed, req.rid))

        def context_of(b):
            return active[b].prompt_ids if active[b] is not None and self.penalize_prompt else None

        def ngram_context_of(b):
            return active[b].prompt_ids if active[b] is not None and self.ngram_prompt else None

        def min_of(b):            # the minimum slot b decodes with: its request's own, else the batcher's; 0 when idle
            req = active[b]
            return 0 if req is None else self.min_new if req.min_new_tokens is None else req.min_new_tokens

        def held(b):              # set_slot's keyword for slot b on a session that carries minimums
            return dict(min_new_tokens=min_of(b)) if sess.seq_row_min is not None else {}

        def guided(b):            # set_slot's keyword for slot b: its request's start state, -1 for a free request or an idle slot
            if self.constraint is None:
                return {}
            req = active[b]
            return dict(constraint_state=-1 if req is None or req.constraint is None else self.constraint_start[req.constraint])

        def room_short(slots):    # does a prompt of these slots hold more distinct tokens than the session reserves?  Then reserve more.
            need = max([len(set(context_of(b) or ())) for b in slots] + [0])
            if not self.penalize_prompt or need <= self._pen_room:
                return False
            self._pen_room = max(32, 1 << (need - 1).bit_length())
            return True

        def ngram_short(slots):   # ... or a longer prompt, or a larger token budget, than the n-gram histories reserve?
            if not self._ng_on:
                return False
            room = max([len(ngram_context_of(b) or ()) for b in slots] + [0])
            # a request is fed its start token, then its tokens round by round: up to a whole round beyond its budget
            fed = max([active[b].max_new_tokens for b in slots if active[b] is not None] + [self.default_new]) + 2 * self.check_every + 2
            if room <= self._ng_room and fed <= self._ng_hist:
                return False
            if room > self._ng_room:
                self._ng_room = max(32, 1 << (room - 1).bit_length())
            self._ng_hist = max(self._ng_hist, fed)
            return True

        def new_session(prev=None, keep=()):
            # (re-)capture the decode step on the cache's current slabs; every slot continues from `state`, the slots in `keep` with the
            # penalty history they had in `prev` (the others start a request: the constructor seeds their context sets)
            start = torch.tensor([s[0] for s in state], dtype=torch.int64)
            pos = torch.tensor([s[2] for s in state], dtype=torch.int64)
            lens_now = list(cache.lens)
            self._room_for([n + self.check_every + 1 for n in lens_now])      # (the session takes the pages of its first round)
            if self.per_request:    # one table row per slot: stream 0, draw 0 (the kept slots take theirs over from `prev` below)
                sampler = dict(row_sampling=[params_of(b) for b in range(B)], row_streams=[0] * B, row_penalties=self._row_pen,
                               logit_bias=self.penalties["logit_bias"])
            else:
                sampler = dict(do_sample=self.do_sample, temperature=self.temperature, seed=seed, top_k=self.top_k, top_p=self.top_p,
                               min_p=self.min_p, no_repeat_ngram_size=self.default_sampling.no_repeat_ngram_size, **self.penalties)
            if self._ng_on:
                sampler.update(ngram_context_ids=[ngram_context_of(b) for b in range(B)], ngram_context_room=self._ng_room,
                               ngram_history=self._ng_hist)
            sampler.update(self.banned)
            if self._min_on:
                sampler.update(min_new_tokens=[min_of(b) for b in range(B)], end_token_id=eos, sequence_row_min=True)
            sn = DecodeSession(m.language_model, cache, start, pos, self.check_every, use_graph=self.use_graph,
                               logprobs=self.want_logprobs, top_logprobs=self.n_top, penalty_context_ids=[context_of(b) for b in range(B)],
                               penalty_context_room=self._pen_room, penalty_history=m.cfg.vocab, constraint=self.constraint,
                               constraint_states=[guided(b)["constraint_state"] for b in range(B)] if self.constraint is not None else None,
                               **sampler)
            if prev is not None:                        # the requests go on: so do their penalty histories and constraint states
                sn.copy_penalty_history(prev, keep)
                sn.copy_constraint_states(prev, keep)
                sn.copy_ngram_history(prev, keep)
                sn.copy_sequence_state(prev, keep)
            cache.lens = lens_now                       # the session only reads them; this loop owns the bookkeeping
            self._grew = False
            return sn
        room_short(range(B))
        ngram_short(range(B))
        sess = new_session()
        while any(r is not None for r in active) or self._other_work():
            if not any(r is not None for r in active):  # only the other kind of work is left (MixedBatcher: flow passes)
                self._between_rounds()
                continue
            k = self.check_every
            if self.paged:      # pages for this round's tokens (the captured step reads the table from device memory; an idle slot, parked
                cfg = m.cfg     # at the start of its segment, keeps one page of its own to write to)
                self._room_for([n + k + 1 for n in cache.lens])
                cache.ensure_tokens([n + k + 1 for n in cache.lens], cfg.kv_heads, cfg.head_dim, self.device)
            sess.rewind_outputs()
            sess.step(k)
            self._between_rounds()                      # (queued behind the decode steps; the host reads the ids after both)
            self.stats["decode_steps"] += k
            ids = sess.pred_ids[:k].cpu()               # [k, B]; the only host sync of the round
            lps = sess.pred_logprobs[:k].cpu() if self.want_logprobs else None
            if self.n_top:
                tids, tlps, rks = sess.pred_top_ids[:k].cpu(), sess.pred_top_logprobs[:k].cpu(), sess.pred_rank[:k].cpu()
            # n-gram histories: a negative length word is a history that ran full and stopped banning (UMV_NGRAM_FULL).  ngram_short sizes
            # the rows so that a live request never gets there - a sizing slip must not pass as a silent loss of the ban.  (An idle slot
            # records its parked start token every step and is started over by the set_slot below every round: check_every entries.)
            if sess.ng_len is not None:
                full = [b for b, n in enumerate(sess.ng_len.tolist()) if n < 0 and active[b] is not None]
                if full:
                    raise RuntimeError(f"the n-gram history of slot(s) {full} ran full: {sess.ng_hist.shape[1]} entries reserved")
            freed = []
            for b in range(B):
                req = active[b]
                if req is None:
                    sess.set_slot(b, bos, 0, 0, **guided(b))         # idle slot: keep it parked at the start of its segment
                    state[b] = (bos, 0, 0)
                    continue
                col = ids[:, b].tolist()
                n_before = len(req.tokens)
                done = False
                for t in col:
                    if t == eos or len(req.tokens) >= req.max_new_tokens:
                        done = True
                        break
                    req.tokens.append(int(t))
                if lps is not None:                     # one value per token emitted this round
                    req.logprobs.extend(lps[:len(req.tokens) - n_before, b].tolist())
                if self.n_top:
                    for s in range(len(req.tokens) - n_before):
                        req.top.append(list(zip(tids[s, b].tolist(), tlps[s, b].tolist())))
                    req.ranks.extend(rks[:len(req.tokens) - n_before, b].tolist())
                if len(req.tokens) >= req.max_new_tokens:
                    done = True
                if not done:
                    cache.lens[b] += k                  # the graph advanced this slot's device counters by k as well
                    state[b] = (col[-1], cache.lens[b], state[b][2] + k)
                    continue
                self._finish(req)
                active[b] = None
                self._free_slot(b)
                if self.queue:
                    active[b] = self.queue.popleft()
                    freed.append(b)
                else:
                    sess.set_slot(b, bos, 0, 0, **guided(b))
                    state[b] = (bos, 0, 0)
            # every slot that was freed this round is refilled by ONE batched prefill (images of the new requests share the
            # ViT and LLM forward; the other slots take part with zero query tokens)
            for b, st in zip(freed, self._prefill_many(freed, [active[b] for b in freed])):
                state[b] = st
            # an admitted request enlarged the cache (new slabs) or brought a prompt longer than the penalty reservation, or a prompt or
            # budget beyond the n-gram histories': new captured step (a list: each of the checks also enlarges its reservation)
            if any([room_short(freed), ngram_short(freed), self._grew]):
                sess = new_session(sess, [b for b in range(B) if b not in freed])
            else:
                for b in freed:
                    row = dict(sampling=params_of(b), stream=0, draw=0) if self.per_request else {}
                    sess.set_slot(b, *state[b], penalty_context_ids=context_of(b), ngram_context_ids=ngram_context_of(b), **row,
                                  **guided(b), **held(b))
        return dict(self.results)

    # ------------------------------------------------------------------ hooks (MixedBatcher)
    def _other_work(self) -> bool:
        return False

    def _free_slot(self, b: int):
        """slot b's request is done: forget its context (a paged cache gets its pages back)"""
        if self.paged:
            self.cache.release(b)
        else:
            self.cache.lens[b] = 0

    def _between_rounds(self):
        pass

    # ------------------------------------------------------------------ internals
    def _prefill(self, b: int, req: _Request):
        """Image(s) then the prompt into slot b (Bagel.chat's order, bagel.py:1321-1392); returns the slot's decode state."""
        if self.prefixes is not None:
            return self._prefill_shared([b], [req])[0]
        m = self.model
        self._free_slot(b)
        view = self.cache.view_segments(b, b + 1)
        view.lens = [0]
        cap = view.cap
        kvl, rope = [0], [0]

        def room(n_ctx):          # growing re-allocates the pooled cache: commit what the view holds, take the view again
            nonlocal view, cap
            self.cache.lens[b] = view.lens[0]
            new_cap = self._check_room(n_ctx, req, cap)
            if new_cap != cap:
                keep = view.lens[0]
                view = self.cache.view_segments(b, b + 1)
                view.lens = [keep]
                cap = view.cap
        for image in req.images:
            gi, kvl, rope = m.prepare_vit_images(kvl, rope, [image], self.image_transform, self.new_token_ids)
            room(kvl[0])
            view = m.forward_cache_update_vit(view, **gi)
        gi, kvl, rope = m.prepare_prompts(kvl, rope, [req.prompt], self.tokenizer, self.new_token_ids)
        if self.penalize_prompt or self.ngram_prompt:
            req.prompt_ids = gi["packed_text_ids"].tolist()[1:-1]        # without the bos / eos wrapper
        room(kvl[0])
        view = m.forward_cache_update_text(view, **gi)
        if view.cap != cap:
            raise RuntimeError("slot view was re-allocated: the request does not fit the reserved capacity")
        self.cache.lens[b] = view.lens[0]
        self.stats["prefills"] += 1
        return (self.new_token_ids["bos_token_id"], view.lens[0], rope[0])

    def _prefill_many(self, slots: List[int], reqs: List[_Request]):
        """Prefill several newly admitted requests together (slots ascending): image j of every request goes through one
        ViT + one packed LLM forward over the WHOLE slot cache, in which the other slots are segments with zero query
        tokens (their keys are not touched: the kernels address the cache by per-token segment / slot indices and skip
        segments without queries).  Falls back to one prefill per request when the requests' image counts differ."""
        if not slots:
            return []
        if len({len(r.images) for r in reqs}) != 1:
            return [self._prefill(b, r) for b, r in zip(slots, reqs)]
        if self.prefixes is not None:
            self.stats["batched_prefills"] = self.stats.get("batched_prefills", 0) + 1
            return self._prefill_shared(slots, reqs)
        # (a single admission takes this path too: on the whole reserved cache its image span replays from a HIP graph,
        # bagel.Bagel.forward_cache_update_vit)
        m, cache, B = self.model, self.cache, self.slots
        cap = cache.cap
        for b in slots:
            self._free_slot(b)
        k = len(slots)
        kvl, rope = [0] * k, [0] * k

        def spread(per_request):          # [k] query lengths -> [B] with zeros for the slots that do not take part
            full = torch.zeros(B, dtype=per_request.dtype)
            full[torch.tensor(slots)] = per_request.cpu()
            return full
        for j in range(len(reqs[0].images)):
            gi, kvl, rope = m.prepare_vit_images(kvl, rope, [r.images[j] for r in reqs], self.image_transform, self.new_token_ids)
            for n, r in zip(kvl, reqs):
                cap = self._check_room(n, r, cap)
            gi["packed_seqlens"] = spread(gi["packed_seqlens"])
            gi["key_values_lens"] = gi["packed_key_value_indexes"] = gi["packed_indexes"] = None   # written for a k-sample cache
            m.forward_cache_update_vit(cache, **gi)
        gi, kvl, rope = m.prepare_prompts(kvl, rope, [r.prompt for r in reqs], self.tokenizer, self.new_token_ids)
        for n, r in zip(kvl, reqs):
            cap = self._check_room(n, r, cap)
        if self.penalize_prompt or self.ngram_prompt:
            for r, ids in zip(reqs, gi["packed_text_ids"].split(gi["text_token_lens"].tolist())):
                r.prompt_ids = ids.tolist()[1:-1]                        # without the bos / eos wrapper
        gi["text_token_lens"] = spread(gi["text_token_lens"])
        gi["key_values_lens"] = gi["packed_key_value_indexes"] = gi["packed_text_indexes"] = None
        m.forward_cache_update_text(cache, **gi)
        if cache.cap != cap:
            raise RuntimeError("the slot cache was re-allocated: a request does not fit the reserved capacity")
        for b, n in zip(slots, kvl):
            assert cache.lens[b] == n
        self.stats["prefills"] += k
        self.stats["batched_prefills"] = self.stats.get("batched_prefills", 0) + 1
        return [(self.new_token_ids["bos_token_id"], n, r) for n, r in zip(kvl, rope)]

    # ------------------------------------------------------------------ share_prefixes
    def _room_for(self, need):
        """share_prefixes: a call is about to take the pages of need[s] tokens per slot - retained prefixes give way, least recently
        used first, until it fits the free list or none is left (then the call fails as it does without sharing).  Off: nothing."""
        if self.prefixes is not None:
            self.prefixes.make_room(self.cache.pages_wanted(need))

    def _prefill_shared(self, slots: List[int], reqs: List[_Request]):
        """_prefill_many with share_prefixes (the requests have the same number of images; a single request takes this path too).
        Chunk j of the group is ONE batched pass over the whole slot cache for the requests that LEAD it (prefix.plan_group); a request
        whose chain is retained adopts the deepest entry before the first pass, a follower copies its leader's slot right after the
        last pass it follows, and both then take part in the passes they do not lead with zero query tokens, as idle slots do.  After
        a pass every leader's context is retained under its prefix key - when the pool has the page for the tail: an entry is a
        convenience, never a reason to fail."""
        m, cache, B, tab, ntid = self.model, self.cache, self.slots, self.prefixes, self.new_token_ids
        cap = cache.cap
        for b in slots:
            self._free_slot(b)
        k, nimg = len(slots), len(reqs[0].images)
        # the prompts are packed once for the keys (and the penalty / n-gram context); the leaders' are packed again at their position
        gi, _, _ = m.prepare_prompts([0] * k, [0] * k, [r.prompt for r in reqs], self.tokenizer, ntid)
        ids = [t.tolist() for t in gi["packed_text_ids"].split(gi["text_token_lens"].tolist())]
        if self.penalize_prompt or self.ngram_prompt:
            for r, t in zip(reqs, ids):
                r.prompt_ids = t[1:-1]                                   # without the bos / eos wrapper
        chains = [chunk_keys(r.images, t, r.image_keys) for r, t in zip(reqs, ids)]
        states, leader = plan_group(chains, tab.__contains__)
        at = [adopt_point(s) for s in states]
        kvl, rope = [0] * k, [0] * k

        def spread(per_request, who):     # query lengths of the requests `who` -> [B] with zeros for every other slot
            full = torch.zeros(B, dtype=per_request.dtype)
            full[torch.tensor([slots[r] for r in who])] = per_request.cpu()
            return full

        def adopt(triples, keep=()):      # [(request, handle, rope position)]: one launch for all the tail copies
            if not triples:
                return
            for r, h, _ in triples:
                self._check_room(h.n, reqs[r], cap)
            tab.make_room(sum(h.tail is not None for _, h, _ in triples), keep)
            cache.adopt_prefix([(slots[r], h) for r, h, _ in triples])
            for r, h, rp in triples:
                kvl[r], rope[r] = h.n, rp
                self.stats["prefix_hits"] += 1
                self.stats["prefix_tokens_reused"] += h.n

        hits = [r for r in range(k) if at[r] >= 0 and states[r][at[r]] == "hit"]
        adopt([(r,) + tab.get(chains[r][:at[r] + 1]) for r in hits], keep={chains[r][:at[r] + 1] for r in hits})
        for j in range(nimg + 1):
            lead = [r for r in range(k) if states[r][j] == "lead"]
            if not lead:
                continue
            at_k, at_r = [kvl[r] for r in lead], [rope[r] for r in lead]
            if j < nimg:
                gi, new_k, new_r = m.prepare_vit_images(at_k, at_r, [reqs[r].images[j] for r in lead], self.image_transform, ntid)
                lens_key, drop = "packed_seqlens", "packed_indexes"
            else:
                gi, new_k, new_r = m.prepare_prompts(at_k, at_r, [reqs[r].prompt for r in lead], self.tokenizer, ntid)
                lens_key, drop = "text_token_lens", "packed_text_indexes"
            for r, n in zip(lead, new_k):
                self._check_room(n, reqs[r], cap)
            gi[lens_key] = spread(gi[lens_key], lead)
            gi["key_values_lens"] = gi["packed_key_value_indexes"] = gi[drop] = None      # written for a cache of the leaders alone
            self._room_for([c + q for c, q in zip(cache.lens, gi[lens_key].tolist())])
            if j < nimg:
                m.forward_cache_update_vit(cache, **gi)
                self.stats["vit_images"] += len(lead)
            else:
                m.forward_cache_update_text(cache, **gi)
            for r, n, p in zip(lead, new_k, new_r):
                kvl[r], rope[r] = n, p
            adopt([(r, cache.live_prefix(slots[leader[r][j]]), rope[leader[r][j]])
                   for r in range(k) if states[r][j] == "follow" and at[r] == j])
            # retain what the pool has a tail page for (after the least recently used entries gave way)
            new = [r for r in lead if chains[r][:j + 1] not in tab]
            tails = [int(kvl[r] % ops.KV_PAGE != 0) for r in new]
            tab.make_room(sum(tails))
            free, keep = len(cache.pool.free), []
            for r, t in zip(new, tails):
                if t <= free:
                    keep.append(r)
                    free -= t
            for r, h in zip(keep, cache.retain_prefix([slots[r] for r in keep])):
                tab.put(chains[r][:j + 1], h, rope[r])
            tab.trim()
        if cache.cap != cap:
            raise RuntimeError("the slot cache was re-allocated: a request does not fit the reserved capacity")
        for b, n in zip(slots, kvl):
            assert cache.lens[b] == n
        self.stats["prefills"] += k
        return [(ntid["bos_token_id"], n, r) for n, r in zip(kvl, rope)]

    def _check_room(self, ctx_tokens: int, req: _Request, cap: int) -> int:
        """Room for `ctx_tokens` of context + the request's new tokens in a slot?  Returns the capacity to go on with: the
        same, or - growable - the enlarged one (the pooled cache is re-allocated HERE, before the forward that would write
        past the old slabs; run() re-captures the decode session afterwards)."""
        need = ctx_tokens + req.max_new_tokens + self.check_every + 1
        if self.paged:          # pages are taken as the context grows; the only bound is the page table's reach
            if need > cap:
                raise ValueError(f"request {req.rid}: {need} tokens of context + answer exceed the page table's reach of {cap}")
            return cap
        if ctx_tokens <= self.max_context and need <= cap:
            return cap
        if not self.growable:
            raise ValueError(f"request {req.rid}: context of {ctx_tokens} tokens exceeds max_context={self.max_context}")
        if self.context_limit is not None and ctx_tokens > self.context_limit:
            raise ValueError(f"request {req.rid}: context of {ctx_tokens} tokens exceeds context_limit={self.context_limit}")
        if need > cap:
            cfg = self.model.cfg
            lens = list(self.cache.lens)
            self.cache.reserved = False
            self.cache.ensure(self.slots, need, cfg.kv_heads, cfg.head_dim, self.model.device)     # >= 2 x the old capacity
            self.cache.reserved = True
            self.cache.lens = lens
            self._grew = True
            self.stats["cache_grows"] += 1
        return self.cache.cap

    def _finish(self, req: _Request):
        bos = self.new_token_ids["bos_token_id"]
        text = self.tokenizer.decode(torch.tensor([bos] + req.tokens, dtype=torch.int64))
        self.results[req.rid] = text.split("<|im_end|>")[0].split("<|im_start|>")[1]   # inferencer.py:277-278
        if self.want_logprobs:
            self.logprobs[req.rid] = list(req.logprobs)
        if self.n_top:
            self.top_logprobs[req.rid] = list(req.top)
            self.ranks[req.rid] = list(req.ranks)
        self.stats["tokens"] += len(req.tokens)


@dataclass
class _T2IRequest:
    rid: int
    prompt: str
    image_shape: Any
    params: tuple              # (num_timesteps, timestep_shift, cfg_text_scale, cfg_img_scale, cfg_interval, renorm_min, renorm_type)
    noise: Optional[torch.Tensor] = None


class MixedBatcher(ContinuousBatcher):
    """VQA decode slots AND text-to-image jobs in one step stream - BASELINE.json configs[4] ("mixed VQA + T2I interleaved
    batch"; with cfg.llm_weight_dtype = "fp8" the decode steps stream the e4m3 images and, with llm_act_dtype = "fp8", the
    flow passes run on the fp8 matrix instruction).

    The reference interleaves understanding and generation inside ONE request's context loop (inferencer.py:552-637: text
    and image items update the context in order, then either gen_text or gen_image runs) and serves one request at a time.
    Here requests of both kinds are in flight together: a round of the serving loop is `check_every` captured decode steps
    for all VQA slots (Bagel.generate_text, bagel.py:1236-1317) followed by `flow_steps_per_round` Euler steps of the active
    text-to-image group (Bagel.generate_image, bagel.py:901-1211: each guided step is one packed forward over the
    conditional / no-text / no-image contexts of every image of the group), all queued on the same stream before the host
    looks at the new token ids.  Retired VQA slots are refilled in flight as in ContinuousBatcher; a finished image group is
    decoded by the VAE in one batch (inferencer.py:234-256) and the next group of queued prompts is admitted.

    Samples are independent rows of every kernel and the two kinds of work share nothing but the weights, so every answer
    and every image equals what the request gets when it is served alone (tests/test_serving_gpu.py, test_fullwidth_gpu.py)."""

    def __init__(self, model, vae_model, tokenizer, new_token_ids, image_transform, slots: int = 8, t2i_batch: int = 4,
                 flow_steps_per_round: int = 2, **kw):
        super().__init__(model, tokenizer, new_token_ids, image_transform, slots=slots, **kw)
        self.vae = vae_model
        self.t2i_batch, self.flow_steps_per_round = int(t2i_batch), int(flow_steps_per_round)
        self.t2i_queue: Deque[_T2IRequest] = deque()
        self._flow = None                 # (FlowSession, [requests]) of the active group
        self.stats.update({"flow_steps": 0, "images": 0, "t2i_groups": 0, "interleaved_rounds": 0})

    def submit_t2i(self, prompt: str, image_shape=(256, 256), num_timesteps: int = 50, timestep_shift: float = 3.0,
                   cfg_text_scale: float = 4.0, cfg_img_scale: float = 1.5, cfg_interval=(0.4, 1.0), cfg_renorm_min: float = 0.0,
                   cfg_renorm_type: str = "global", init_noise: Optional[torch.Tensor] = None) -> int:
        """Queue a text-to-image request (the defaults are interactive_image_generator.py:303-306's).  init_noise (optional,
        [h*w, patch*patch*z]) fixes the starting latent; otherwise it is drawn from torch's CPU generator at admission,
        as the reference does (bagel.py:893)."""
        rid = self._next_id
        self._next_id += 1
        params = (int(num_timesteps), float(timestep_shift), float(cfg_text_scale), float(cfg_img_scale),
                  tuple(float(v) for v in cfg_interval), float(cfg_renorm_min), str(cfg_renorm_type))
        self.t2i_queue.append(_T2IRequest(rid, prompt, tuple(int(v) for v in image_shape), params, init_noise))
        return rid

    # ------------------------------------------------------------------ the flow side of a round
    def _other_work(self) -> bool:
        return self._flow is not None or bool(self.t2i_queue)

    def _admit_t2i(self):
        """The next group: up to t2i_batch queued prompts with the same image shape and sampler parameters."""
        first = self.t2i_queue[0]
        group, rest = [], deque()
        while self.t2i_queue:
            r = self.t2i_queue.popleft()
            if len(group) < self.t2i_batch and r.image_shape == first.image_shape and r.params == first.params:
                group.append(r)
            else:
                rest.append(r)
        self.t2i_queue = rest
        m, ntid, n = self.model, self.new_token_ids, len(group)
        steps, shift, s_text, s_img, interval, rmin, rtype = first.params
        shapes = [first.image_shape] * n
        # gen context = the prompt; no-text context = empty; no-image context = the prompt again (inferencer.py:583-607)
        gen = NaiveCache(m.cfg.layers)
        gi, kvl, rope = m.prepare_prompts([0] * n, [0] * n, [r.prompt for r in group], self.tokenizer, ntid)
        gen = m.forward_cache_update_text(gen, **gi)
        gl = m.prepare_vae_latent(kvl, rope, shapes, ntid)
        if any(r.noise is not None for r in group):
            parts = list(gl["packed_init_noises"].split([gl["packed_init_noises"].shape[0] // n] * n))
            for j, r in enumerate(group):
                if r.noise is not None:
                    parts[j] = r.noise.to(parts[j].dtype).reshape(parts[j].shape)
            gl["packed_init_noises"] = torch.cat(parts, 0)
        gt = m.prepare_vae_latent_cfg([0] * n, [0] * n, shapes)
        gim = m.prepare_vae_latent_cfg(kvl, rope, shapes)
        from .bagel import FlowSession
        args = dict(gl)
        args.update(dict(
            past_key_values=gen, key_values_lens=gl.get("key_values_lens"), num_timesteps=steps, timestep_shift=shift,
            cfg_renorm_min=rmin, cfg_renorm_type=rtype, cfg_interval=interval, cfg_text_scale=s_text, cfg_img_scale=s_img,
            cfg_text_past_key_values=NaiveCache(m.cfg.layers), cfg_text_packed_position_ids=gt["cfg_packed_position_ids"],
            cfg_img_past_key_values=gen.snapshot(), cfg_img_packed_position_ids=gim["cfg_packed_position_ids"]))
        self._flow = (FlowSession(m, args), group)
        self.stats["t2i_groups"] += 1

    def _between_rounds(self):
        if self._flow is None:
            if not self.t2i_queue:
                return
            self._admit_t2i()
        flow, group = self._flow
        before = flow.i
        flow.step(self.flow_steps_per_round)
        self.stats["flow_steps"] += flow.i - before
        self.stats["interleaved_rounds"] += 1
        if flow.finished:
            m = self.model
            lats = list(flow.latents())
            px = self.vae.decode_tokens_batch_to_uint8(lats, group[0].image_shape, m.latent_downsample, m.latent_patch_size)
            for j, r in enumerate(group):
                self.results[r.rid] = px[j].cpu()
                self.latents[r.rid] = lats[j].clone()
            self.stats["images"] += len(group)
            self._flow = None

    def run(self):
        """Serve everything submitted: {request id: answer text | uint8 [H, W, 3] image}; self.latents keeps the final latent
        tokens of every image (tests compare them with the requests served alone)."""
        self.latents: Dict[int, torch.Tensor] = {}
        if self.queue:
            return super().run()
        with torch.no_grad(), ops.device_scope(self.device):
            while self._other_work():          # no VQA request at all: only image groups
                self._between_rounds()
        return dict(self.results)
