"""Beam search decode (include/unimedvl_hip.h, "beam search decode").

K beams of B requests are R = B * K ordinary rows of the decode step - every row its own segment of a forked paged cache
(kvcache.PagedCache.fork_beams: the beams share the prompt's pages) - through DecodeSession's layer loop, one copy of it.  The step
ends with three launches instead of the plain step end: the rows' candidate lists, the per-request step end (order, walk, finished
list, done word, back-pointers, counters, page-table rows, copy list) and the copy of the partially filled pages.  One HIP graph per
step, no host round trip but the done words every few steps; the host rebuilds the sequences from the back-pointers at the end.
"""
import os

import torch

from . import ops
from .decode import DecodeSession

# what a beam search does not combine with, by keyword -> the value that leaves it off (speculative decode's precedent: refused by
# ValueError before any launch).  State that would have to follow the parent beam - penalty counts, n-gram histories, constraint
# states - is the follow-up of DESIGN.md section 7.
BEAM_EXCLUDES = dict(do_sample=False, sampling=None, draft_len=0, forced_ids=None, top_logprobs=0, return_logits=False, constraint=None,
                     choices=None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None,
                     no_repeat_ngram_size=0, top_k=0, top_p=1.0, min_p=0.0)


def check_beam_keywords(num_beams, **kw):
    """ValueError where num_beams > 1 meets a keyword it excludes (kw: name -> value; names outside BEAM_EXCLUDES are a TypeError),
    or the unfused step end (UMV_DECODE_FUSED_ARGMAX=0)."""
    unknown = set(kw) - set(BEAM_EXCLUDES)
    if unknown:
        raise TypeError(f"check_beam_keywords: unknown keywords {sorted(unknown)}")
    if num_beams <= 1:
        return
    on = [k for k, v in kw.items() if not _is_off(v, BEAM_EXCLUDES[k])]
    if on:
        raise ValueError(f"num_beams > 1 (beam search decode) excludes {', '.join(sorted(on))}")
    if os.environ.get("UMV_DECODE_FUSED_ARGMAX", "1") in ("0", ""):
        raise ValueError("num_beams > 1 (beam search decode) rides on the fused step end: UMV_DECODE_FUSED_ARGMAX must not be 0")


def _is_off(value, neutral):
    if isinstance(value, (list, tuple)):                 # one value per sample
        return all(_is_off(v, neutral) for v in value)
    if neutral is None:
        return value is None or value == {}
    return value == neutral


def check_beam_options(num_beams, length_penalty, early_stopping, num_return_sequences):
    """(length_penalty as float, early_stopping as bool, num_return_sequences as int); ValueError for what is none of these"""
    if isinstance(early_stopping, str) or early_stopping not in (True, False):
        raise ValueError(f"early_stopping must be True or False (HF's \"never\" is not available), got {early_stopping!r}")
    lp = float(length_penalty)
    if lp != lp or lp in (float("inf"), float("-inf")):
        raise ValueError(f"length_penalty must be finite, got {length_penalty!r}")
    n = num_return_sequences
    if isinstance(n, bool) or int(n) != n or not 1 <= n <= max(1, num_beams):
        raise ValueError(f"num_return_sequences must be an integer in [1, num_beams = {num_beams}], got {n!r}")
    return lp, bool(early_stopping), int(n)


class BeamDecodeSession(DecodeSession):
    """A DecodeSession over cache.fork_beams(num_beams, max_length + 1) with B * num_beams samples and logprobs=True.  `cache` is the
    prefilled PagedCache of the B requests; it is read, never written: release() gives the fork's pages back and leaves it as it
    was.  start_tokens / positions: one per request.  run() steps until every request is done or max_length steps are taken;
    result() returns, per request, up to num_return_sequences hypotheses, best first.  num_beams = 1 builds the plain DecodeSession
    over `cache` itself (greedy decode)."""

    def __new__(cls, llm, cache, start_tokens, positions, max_length, num_beams=1, **kw):
        if ops.check_beams(num_beams) == 1:
            for k in ("length_penalty", "early_stopping", "num_return_sequences", "eos_check_every"):
                kw.pop(k, None)
            if not kw.get("min_new_tokens"):            # (the plain session takes the end token only to hold it back)
                kw.pop("end_token_id", None)
            return DecodeSession(llm, cache, start_tokens, positions, max_length, **kw)
        return super().__new__(cls)

    def __init__(self, llm, cache, start_tokens, positions, max_length, num_beams=1, *, end_token_id=None, length_penalty=1.0,
                 early_stopping=False, num_return_sequences=1, use_graph=True, nsplit=None, eos_check_every=8, bad_words_ids=None,
                 suppress_tokens=None, begin_suppress_tokens=None, min_new_tokens=0, **excluded):
        check_beam_keywords(num_beams, **excluded)
        if not hasattr(cache, "fork_beams"):
            raise ValueError(f"num_beams > 1 needs a PagedCache (the beams share the prompt's pages), got {type(cache).__name__}")
        if max_length < 1:
            raise ValueError(f"beam search decode needs max_length >= 1, got {max_length}")
        K = ops.check_beams(num_beams, llm.cfg.vocab, len(cache.lens))
        self.length_penalty, self.early_stopping, self.num_return_sequences = check_beam_options(K, length_penalty, early_stopping,
                                                                                                 num_return_sequences)
        self.end_token_id = None if end_token_id is None else int(end_token_id)
        self.K, self.requests, self.eos_check_every = K, len(cache.lens), max(1, int(eos_check_every))
        with ops.device_scope(llm.device):
            fork = cache.fork_beams(K, max_length + 1)
            try:
                starts = torch.as_tensor(start_tokens).reshape(-1).repeat_interleave(K)
                pos = torch.as_tensor(positions).reshape(-1).repeat_interleave(K)
                self._init(llm, fork, starts, pos, max_length, use_graph=False, nsplit=nsplit, logprobs=True)
                self.beam = ops.BeamState(self.requests, K, max_length, self.dev, self.length_penalty)
                # banned sequences (the first logit stage under beams: its state is the step number and the back-pointers): min_new_tokens
                # one per request; the start tokens are kept aside, ids moves on
                self._init_sequences(bad_words_ids, suppress_tokens, begin_suppress_tokens, min_new_tokens, self.end_token_id, beams=K)
                if self.seq_table is not None:
                    self.seq_start = torch.as_tensor(start_tokens).reshape(-1).to(device=self.dev, dtype=torch.int64).clone()
                    self.seq_beam = (self.beam.beam_tok, self.beam.beam_parent, self.step_idx, self.seq_start, K)
                self.pools = ops.beam_pool_pointers(fork.pool.slabs)
                if use_graph:
                    self._capture()
            except Exception:
                fork.release_all()
                raise

    def _step_end(self):
        """the three launches that end a beam step, instead of the pick and the bookkeeping of the plain step end"""
        st, c = self.beam, self.cache
        ops.beam_candidates(self.logits, self.lse_part, st.cand_ids, st.cand_lp, st.rank)
        ops.beam_step_end(self.tok_slot, self.tok_pos, self.kv_len, self.ids, self.step_idx, st, c.pool.table, c.beam_own, c.beam_j0,
                          self.end_token_id, self.early_stopping)
        ops.beam_kv_copy(st.copies, self.pools, c.pool.slabs)

    def _state(self):
        # ... and the scores, the finished lists, the done words, the copy list and the table rows: the warm-up step before the
        # capture leaves no trace (what it copied went into spare pages, whose contents nothing reads before a later copy)
        return super()._state() + self.beam.written() + (self.cache.pool.table,)

    @ops.on_device
    def done(self):
        """the requests' done words (a host read)"""
        return [bool(v) for v in self.beam.hdr[:, 2].cpu().tolist()]

    @ops.on_device
    def run(self):
        """Step until every request is done or max_length steps are taken; the done words are read every eos_check_every steps."""
        while self.steps_done < self.max_length:
            self.step(min(self.eos_check_every, self.max_length - self.steps_done))
            if all(self.done()):
                break
        return self

    @ops.on_device
    def result(self):
        """Per request a list of up to num_return_sequences hypotheses, best first (score descending, the earlier entry among
        equals): dicts with tokens (the end token included where the hypothesis ended on it), tokens_no_end, score (the normalised
        one), total (the raw sum of log-probabilities) and logprobs (one per token).  Before a request is done or max_length is
        reached its list holds only what has finished so far."""
        st, K = self.beam, self.K
        hdr, fin_f, fin_i = st.hdr.cpu(), st.fin_f.cpu(), st.fin_i.cpu()
        tok = st.beam_tok.cpu().reshape(self.max_length, self.requests, K)
        par = st.beam_parent.cpu().reshape(self.max_length, self.requests, K)
        blp = st.beam_lp.cpu().reshape(self.max_length, self.requests, K)
        out = []
        for b in range(self.requests):
            n = int(hdr[b, 0])
            order = sorted(range(n), key=lambda s: (-float(fin_f[b, s, 0]), int(fin_i[b, s, 3])))
            hyps = []
            for s in order[:self.num_return_sequences]:
                t, beam, last, _ = (int(v) for v in fin_i[b, s])
                toks, lps = [last], [float(fin_f[b, s, 2])]
                for u in range(t - 1, -1, -1):           # the back-pointers: nothing was reordered on the device but KV
                    toks.append(int(tok[u, b, beam]))
                    lps.append(float(blp[u, b, beam]))
                    beam = int(par[u, b, beam])
                toks.reverse()
                lps.reverse()
                hyps.append(dict(tokens=toks, tokens_no_end=toks[:-1] if toks[-1] == self.end_token_id else toks,
                                 score=float(fin_f[b, s, 0]), total=float(fin_f[b, s, 1]), logprobs=lps))
            out.append(hyps)
        return out

    def commit(self, steps=None):
        raise RuntimeError("a beam session decodes on a throwaway fork: there is nothing to commit (release() returns its pages)")

    def set_slot(self, *a, **kw):
        raise RuntimeError("a beam session's rows belong to its requests' beams: set_slot is not available")

    def release(self):
        """Return the fork's pages to the pool (each exactly once, by the host lists).  The session is finished."""
        self.graph = None
        self.cache.release_all()


def beam_generate(llm, cache, start_tokens, positions, max_length, num_beams, *, end_token_id=None, length_penalty=1.0,
                  early_stopping=False, num_return_sequences=1, use_graph=True, eos_check_every=8, bad_words_ids=None,
                  suppress_tokens=None, begin_suppress_tokens=None, min_new_tokens=0):
    """One beam search over `cache` (a prefilled PagedCache, left as it was): the session's result().  bad_words_ids, suppress_tokens,
    begin_suppress_tokens, min_new_tokens (an int or one per request): DecodeSession's keywords of these names, per beam."""
    sess = BeamDecodeSession(llm, cache, start_tokens, positions, max_length, num_beams, end_token_id=end_token_id,
                             length_penalty=length_penalty, early_stopping=early_stopping, num_return_sequences=num_return_sequences,
                             use_graph=use_graph, eos_check_every=eos_check_every, bad_words_ids=bad_words_ids,
                             suppress_tokens=suppress_tokens, begin_suppress_tokens=begin_suppress_tokens, min_new_tokens=min_new_tokens)
    try:
        return sess.run().result()
    finally:
        sess.release()
