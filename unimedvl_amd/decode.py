"""Greedy KV-cache decode with all bookkeeping on the device.

The reference loop (codes/modeling/unimedvl/bagel.py:1262-1314) rebuilds its index
tensors with .tolist() splits every step, re-merges the whole KV tensor in every layer
and syncs with the host three times per token.  Here one decode step is a fixed kernel
sequence over static buffers (embed -> rmsnorm -> 28 x [QKV GEMM, fused q/k-norm + RoPE +
KV append + split-KV attention, combine, o_proj + residual, rmsnorm, SwiGLU GEMM,
down + residual, next rmsnorm] -> lm_head -> argmax -> advance), captured once into a HIP
graph and replayed; slot, position and kv_len counters live in device memory
(umv_decode_advance).

Each of the three N = 3584 / 4608 GEMMs (QKV, o, down) can run split along K ("split-K"): fp32 partial
sums that the kernel which follows anyway finishes - the attention kernel (or umv_qkv_post) sums the QKV
partials, umv_residual_rmsnorm_bf16 = partial sum + residual add + the next RMSNorm - so a split never
adds a launch and the summation order stays fixed.

Tried and measured slower on MI355X, no longer wired in here (profiles/HISTORY.md section 5b): RMSNorm folded into the next
GEMM's prologue (norm_w of umv_gemm_bf16: every workgroup pays the normalise + stage latency before its
first MFMA, step 3.40 -> 3.93 ms) and weight prefetch into the Infinity Cache on a parallel graph branch
(umv_prefetch: the branch does not overlap under graph replay, 3.43 -> 4.5-5.4 ms).
"""
import os

import torch

from . import _lib, ops
from . import sampling as sampling_mod
from .kvcache import NaiveCache

BF16 = torch.bfloat16


def _lib_flag(word):
    """a count-table flag word (unsigned 32 bit) as the int32 torch stores"""
    return word - (1 << 32) if word & 0x80000000 else word


class DecodeSession:
    draft_len = 0       # tokens a step verifies per sample besides its input (speculative.SpeculativeDecodeSession): a step has B * (draft_len + 1) rows

    def __init__(self, llm, cache: NaiveCache, start_tokens, positions, max_length, use_graph=True, nsplit=None,
                 do_sample=False, temperature=1.0, seed=0, logprobs=False, forced_ids=None, *,
                 repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None, penalty_context_ids=None,
                 penalty_context_room=None, penalty_history=None, row_sampling=None, row_streams=None, row_penalties=False,
                 top_logprobs=0, constraint=None, constraint_states=None, no_repeat_ngram_size=0, ngram_context_ids=None,
                 ngram_context_room=None, ngram_history=None, bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None,
                 min_new_tokens=0, end_token_id=None, sequence_row_min=False, top_k=0, top_p=1.0, min_p=0.0):
        """logprobs: also record pred_logprobs (fp32 [max_length, B]) - row s is the log-probability of in_ids[s + 1], the token step s
        picked (include/unimedvl_hip.h, token log-probabilities: of softmax(logits) in greedy decoding, of softmax(bf16(logits / T))
        when sampling).  forced_ids (int64 [max_length, B]): where an entry is >= 0 that token is fed to the next step instead of the
        pick - pred_ids still records the pick, pred_logprobs the forced token's value; negative = free-running.  Implies logprobs.
        Both ride on the fused step end: B <= 64 and UMV_DECODE_FUSED_ARGMAX not 0, ValueError otherwise.
        top_k / top_p / min_p (0 / 1.0 / 0.0 = off): truncated sampling (include/unimedvl_hip.h) - they need do_sample and, like
        logprobs, the fused step end.  With one on, the step ends with umv_decode_step_end_truncated - still two launches after the last
        norm, still one graph - and pred_cut_y (fp32) / pred_n_kept (int32), both [max_length, B], record each step's cutoff value and
        kept-column count.  pred_logprobs stay those of the untruncated softmax.  All off: today's step, launch for launch.
        repetition_penalty / presence_penalty / frequency_penalty (1.0 / 0.0 / 0.0 = off) and logit_bias ({token: float}, -inf bans a
        token): the logit penalties of include/unimedvl_hip.h - one umv_logit_penalty_bf16 launch between the lm_head call and the step
        end rewrites the stored logits of the columns a sample has generated (the tokens fed at steps 1.., forced ones included), of its
        context set and of the biased columns, and the tiles' keys and statistics with them; greedy and sampled picks, pred_logprobs,
        truncation and `logits` are all those of the ADJUSTED logits.  penalty_context_ids: per sample a list of tokens (the prompt)
        that count as seen for the repetition penalty.  The session owns the history: set_slot resets a slot's, rewind_outputs keeps
        it.  penalty_context_room: context tokens per slot to reserve for later set_slot calls (default: the longest list given) -
        keep it at what the prompts need: the kernel walks the whole reservation of every row at every step;
        penalty_history: distinct generated tokens per slot to reserve (default max_length - more when requests outlive a round of
        max_length steps).  All neutral: today's step, launch for launch, no buffer allocated.  Works on the unfused step too.
        row_sampling (a list of B sampling.SamplingParams): per-row sampling parameters (include/unimedvl_hip.h) - every sample decodes
        with its OWN sampler, penalties and sampling key inside the one captured step: the session owns a table of B 48-byte rows in
        device memory, the lm_head epilogue, the penalty kernel and umv_decode_step_end_rows read it.  Excludes the scalar keywords
        above (do_sample, temperature, top_k / top_p / min_p, the three penalties); `seed` is the seed of the rows whose params carry
        none, logit_bias stays session-wide.  row_streams: the `stream` word of every row's key (default: the row index - the scalar
        session's keying); a row's draw counter starts at 0, advances by one per step and is NOT rewound by rewind_outputs.
        set_slot(b, ..., sampling=, stream=, draw=) gives a slot new parameters between replays without a re-capture.  pred_cut_y /
        pred_n_kept are always recorded (a row without a filter: -inf / vocab).  The penalty buffers are allocated only if a row is
        not neutral, a bias is given, or row_penalties=True reserves them for later set_slot calls.  Rides on the fused step end
        (B <= 64).  Without row_sampling nothing is allocated and the step is today's, launch for launch.
        top_logprobs (n, 0 = off, at most 20): also record, per step, the n most likely tokens with their log-probabilities and the rank
        of the token fed next (include/unimedvl_hip.h, top-n alternative tokens) - pred_top_ids (int32) / pred_top_logprobs (fp32),
        both [max_length, B, n], and pred_rank (int32 [max_length, B]); row s belongs to in_ids[s + 1] like pred_logprobs.  One
        umv_decode_top_logprobs launch behind the step end, in the same graph; implies logprobs.  The alternatives are those of the
        untruncated softmax of the stored (adjusted) logits, whatever sampler, filters, penalties or forced tokens the step runs with.
        Off: nothing is allocated, nothing is launched.
        constraint (a constraints.TokenAutomaton): constrained decoding (include/unimedvl_hip.h, token automata) - every sample carries
        a state word on the device; one umv_logit_constrain_bf16 launch behind the lm_head call (and the penalty kernel) masks the
        stored logits of a sample to the tokens its state has an edge for, and one umv_constraint_advance launch at the very end of the
        step moves the word along the token that will be fed next - the pick, or the forced token.  Picks, pred_logprobs (those of the
        softmax renormalised over the allowed set), truncation, top_logprobs and `logits` are all those of the masked logits.
        constraint_states: one start state per sample (default: state 0 for all), -1 leaves a sample free - its step is today's, bit
        for bit.  The session owns the device tables and the words: set_slot(constraint_state=) rewrites one, rewind_outputs keeps
        them.  Works on the fused and the unfused step and with every keyword above; not with draft_len > 0 (ValueError).  None:
        today's step, launch for launch, no buffer allocated.
        no_repeat_ngram_size (n, 0 = off, at most 16; an int, or a list of one per sample): no sample is fed a token that would repeat
        an n-gram of its history (include/unimedvl_hip.h, no-repeat n-grams; HF's NoRepeatNGramLogitsProcessor) - one
        umv_logit_ngram_ban_bf16 launch behind the lm_head call and the penalty kernel, before the constraint mask, records the token
        the step is fed and sets the banned columns of the stored logits to -inf, their tiles' keys and statistics with them; picks,
        pred_logprobs, truncation, top_logprobs and `logits` are those of the banned logits.  With row_sampling a row's size is its
        SamplingParams.no_repeat_ngram_size and the scalar keyword stays 0.  ngram_context_ids: per sample the tokens that precede
        the start token in its history (the prompt; negative entries are separators nothing matches) - default: generated tokens only.
        The session owns the history: set_slot starts a slot's over, rewind_outputs keeps it.  ngram_context_room: context tokens per
        slot to reserve for later set_slot calls (default: the longest list given); ngram_history: fed tokens per slot to reserve
        (default max_length - more when requests outlive a round of max_length steps; with row_sampling, giving it reserves the
        buffers even while every row's size is 0).  A slot whose history runs full stops banning.  Works on the fused and the unfused
        step and with every keyword above; not with draft_len > 0 (ValueError).  Off: today's step, launch for launch, no buffer
        allocated.
        bad_words_ids (a list of token lists of at most 16), suppress_tokens, begin_suppress_tokens (token lists) and min_new_tokens
        (an int, or a list of one per sample; needs end_token_id): HF's keywords of these names (include/unimedvl_hip.h, banned
        sequences) - no sample is fed the last token of a bad word whose other tokens it was just fed, a suppressed token, a
        begin-suppressed token as its first pick, or end_token_id among its first min_new_tokens picks.  One
        umv_logit_sequence_ban_bf16 launch behind the n-gram ban and before the constraint mask records the token the step is fed in
        the sample's count and 15-token tail and sets the banned columns to -inf, their tiles' keys and statistics with them.  The
        history is the fed tokens, start token first: a bad word that begins in the prompt is not seen.  The session owns the state:
        set_slot starts a slot's over (min_new_tokens= gives it its own minimum), rewind_outputs keeps it, copy_sequence_state takes
        another session's.  sequence_row_min=True (with end_token_id) reserves the end-token entry and the per-slot minimums for later
        set_slot calls while every minimum is 0.  Works on the fused and the unfused step and with every keyword above; not with
        draft_len > 0 (ValueError).  Off: today's step, launch for launch, no buffer allocated."""
        if constraint is None and constraint_states is not None:
            raise ValueError("constraint_states goes with constraint")
        if constraint is not None and self.draft_len:
            raise ValueError("constraint is not available with draft_len > 0 (speculative decode)")
        if row_sampling is not None:
            scalar = sampling_mod.off_neutral(locals())
            if scalar:
                raise ValueError(f"row_sampling excludes the scalar sampler keywords (got {scalar})")
        elif row_streams is not None or row_penalties:
            raise ValueError("row_streams / row_penalties go with row_sampling")
        top_logprobs = ops.check_top_logprobs(top_logprobs, llm.cfg.vocab)
        if top_logprobs and self.draft_len:
            raise ValueError("top_logprobs is not available with draft_len > 0 (speculative decode)")
        with ops.device_scope(llm.device):
            self._init(llm, cache, start_tokens, positions, max_length, use_graph=use_graph, nsplit=nsplit, do_sample=do_sample,
                       temperature=temperature, seed=seed, logprobs=logprobs, forced_ids=forced_ids,
                       repetition_penalty=repetition_penalty, presence_penalty=presence_penalty, frequency_penalty=frequency_penalty,
                       logit_bias=logit_bias, penalty_context_ids=penalty_context_ids, penalty_context_room=penalty_context_room,
                       penalty_history=penalty_history, row_sampling=row_sampling, row_streams=row_streams, row_penalties=row_penalties,
                       top_logprobs=top_logprobs, constraint=constraint, constraint_states=constraint_states, top_k=top_k, top_p=top_p,
                       min_p=min_p, no_repeat_ngram_size=no_repeat_ngram_size, ngram_context_ids=ngram_context_ids,
                       ngram_context_room=ngram_context_room, ngram_history=ngram_history, bad_words_ids=bad_words_ids,
                       suppress_tokens=suppress_tokens, begin_suppress_tokens=begin_suppress_tokens, min_new_tokens=min_new_tokens,
                       end_token_id=end_token_id, sequence_row_min=sequence_row_min)

    @property
    def device(self):
        return self.dev

    def _init(self, llm, cache, start_tokens, positions, max_length, *, use_graph, nsplit=None, do_sample=False, temperature=1.0, seed=0,
              logprobs=False, forced_ids=None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None,
              penalty_context_ids=None, penalty_context_room=None, penalty_history=None, row_sampling=None, row_streams=None,
              row_penalties=False, top_logprobs=0, constraint=None, constraint_states=None, top_k=0, top_p=1.0, min_p=0.0,
              no_repeat_ngram_size=0, ngram_context_ids=None, ngram_context_room=None, ngram_history=None, bad_words_ids=None,
              suppress_tokens=None, begin_suppress_tokens=None, min_new_tokens=0, end_token_id=None, sequence_row_min=False):
        """the constructor's keywords under the constructor's names, already checked against each other (__init__)"""
        cfg, dev = llm.cfg, llm.device
        self.llm, self.cache, self.cfg, self.dev = llm, cache, cfg, dev
        B = len(cache.lens)
        self.B = B
        self.max_length = max_length
        # a step's rows: one per sample, or - with drafts to verify - draft_len + 1 per sample, sample after sample, at consecutive
        # slots and positions; every buffer and routing rule below that went by the sample count goes by the row count R
        k = self.draft_len
        R = self.rows = B * (k + 1)
        nq, nkv, hd, H = cfg.heads, cfg.kv_heads, cfg.head_dim, cfg.hidden
        if hasattr(cache, "ensure_tokens"):      # paged cache: pages for every slot's own decode horizon (the captured step reads the table)
            cache.ensure_tokens([n + max_length + 1 + k for n in cache.lens], nkv, hd, dev)
        else:
            cache.ensure(B, max(cache.lens) + max_length + 1 + k, nkv, hd, dev)
        self.lens0 = list(cache.lens)
        i32 = dict(dtype=torch.int32, device=dev)

        def per_row(t):      # a per-sample vector -> per row, the row's offset inside its sample added
            return t if k == 0 else t.repeat_interleave(k + 1) + torch.arange(k + 1, dtype=t.dtype, device=t.device).repeat(B)
        self.ids = start_tokens.to(device=dev, dtype=torch.int64).clone()
        if k:
            self.ids = self.ids.repeat_interleave(k + 1)
        self.tok_seg = torch.arange(B, **i32) if k == 0 else torch.arange(B, **i32).repeat_interleave(k + 1)
        self.tok_slot = per_row(torch.tensor(cache.lens, dtype=torch.int32).to(dev))
        pmax = int(positions.max()) if positions.numel() else 0
        if (int(positions.min()) if positions.numel() else 0) < 0 or pmax + max_length + k >= cfg.max_position:
            raise ValueError(f"decode would reach rope position {pmax + max_length + k} >= max_position_embeddings {cfg.max_position}")
        self.tok_pos = per_row(positions.to(device=dev, dtype=torch.int32).clone())
        self.kv_len = torch.tensor(cache.lens, dtype=torch.int32).to(dev) + (k + 1)
        self.cu_q = torch.arange(B + 1, **i32) * (k + 1)
        self.in_ids = torch.zeros((max_length, B), dtype=torch.int64, device=dev)    # token fed at each step
        self.pred_ids = torch.zeros((max_length, B), dtype=torch.int64, device=dev)  # token predicted at each step
        if max_length > 0 and k == 0:       # (a session with drafts logs its tokens per sample: out_ids / n_out)
            self.in_ids[0].copy_(self.ids)
        # step counter(s): entry 0 is THE counter (sampling, the unfused step end); the fused argmax step end keeps one per sample
        # so that its workgroups share no word (umv_decode_step_end_argmax)
        self.step_idx = torch.zeros(max(B, 1), dtype=torch.int64, device=dev)
        max_kv = max(cache.lens) + max_length + 1 + k
        # split the key range so that every wavefront walks ~2 blocks of 32 keys (latency bound otherwise)
        if nsplit is None and os.environ.get("UMV_DECODE_NSPLIT"):
            nsplit = int(os.environ["UMV_DECODE_NSPLIT"])   # tuning only
        # ... but no more than ~1024 waves in all: with many samples the partial (O, m, l) traffic and the combine grow with the
        # split count (B = 32, context 1156: 4.45 ms per step at 8 splits, 4.53 at 19; B = 8 is unchanged by the cap)
        # round 4 (single-wave workgroups; profiles/r04_decode_nsplit_sweep.txt): B = 32, context 1156: 6 splits 4.009 ms, 8 splits 4.061,
        # 4 splits 4.046, 12 splits 4.064; B = 8, context 1060: 24 splits 3.116, 17 splits 3.125, 28 splits 3.131 -> ~768 waves at
        # 9 .. 32 samples (1024 otherwise: unmeasured, unchanged) and ~48 keys per split up to 8 samples
        if nsplit is None:
            keys = 48 if R <= 8 else 64
            nsplit = max(1, min(32, (max_kv + keys - 1) // keys, max(1, (768 if 8 < R <= 32 else 1024) // (R * nkv))))
        self.nsplit = nsplit
        # waves per attention workgroup splitting its key range with an LDS merge (umv_attn_args.wave_split: 0 = single-wave workgroups);
        # UMV_DECODE_WSPLIT=2|4 for the A/B of profiles/r06_decode_wave_split.txt
        self.wave_split = int(os.environ.get("UMV_DECODE_WSPLIT", "0") or 0)
        self.ws = ops.attn_workspace(B, nq, hd, k + 1, self.nsplit, dev) if self.nsplit > 1 else None
        self.max_kv = max_kv
        # static activations
        self.seq = torch.empty((R, H), dtype=BF16, device=dev)
        self.x = torch.empty((R, H), dtype=BF16, device=dev)
        self.qkv = torch.empty((R, (nq + 2 * nkv) * hd), dtype=BF16, device=dev)
        self.q = torch.empty((R, nq, hd), dtype=BF16, device=dev)
        self.o = torch.empty((R, nq * hd), dtype=BF16, device=dev)
        self.act = torch.empty((R, cfg.inter), dtype=BF16, device=dev)
        self.hn = torch.empty((R, H), dtype=BF16, device=dev)
        self.logits = torch.empty((R, cfg.vocab), dtype=BF16, device=dev)
        # greedy: the argmax rides on the lm_head epilogue (one key per 16-column tile and row) and is finished by the
        # step-end kernel - the separate 25 us argmax launch over the logits is gone (UMV_DECODE_FUSED_ARGMAX=0 restores it)
        # sampling rides the same way (round 5): the keys order bf16(logit / T) + Gumbel noise, their maximum is one draw from the softmax -
        # the sampled step has the greedy step's two-launch tail (lm_head -> sample -> step_end was 3.29 ms against 3.12)
        self.fused_argmax = R <= 64 and os.environ.get("UMV_DECODE_FUSED_ARGMAX", "1") not in ("0", "")
        if self.fused_argmax:
            self.amax_part = torch.zeros((R, (cfg.vocab + 15) // 16), dtype=torch.int64, device=dev)

        def need_fused(what):
            if not self.fused_argmax:
                raise ValueError(f"{what} ride on the fused step end: at most 64 samples and UMV_DECODE_FUSED_ARGMAX not 0 "
                                 f"(got B={B}, UMV_DECODE_FUSED_ARGMAX={os.environ.get('UMV_DECODE_FUSED_ARGMAX', '1')!r})")
        # token log-probabilities / forced tokens: the lm_head epilogue also leaves the softmax statistics of every tile, and the step
        # ends with umv_decode_step_end_logprob instead - same launch count, still one graph
        self.top_logprobs = int(top_logprobs)
        self.logprobs = bool(logprobs) or forced_ids is not None or self.top_logprobs > 0
        self.forced_ids = self.pred_logprobs = self.lse_part = None
        if self.logprobs:
            need_fused("logprobs / forced_ids")
            if forced_ids is not None:
                f = torch.as_tensor(forced_ids, dtype=torch.int64)
                if tuple(f.shape) != (max_length, B):
                    raise ValueError(f"forced_ids must be [max_length, B] = [{max_length}, {B}], got {tuple(f.shape)}")
                if f.numel() and int(f.max()) >= cfg.vocab:
                    raise ValueError(f"forced_ids holds token {int(f.max())} >= vocab {cfg.vocab}")
                self.forced_ids = f.to(dev).contiguous()
            # (one tile statistic per ROW; a session with drafts logs per sample: out_logprobs, speculative.py)
            self.lse_part = torch.zeros((R, (cfg.vocab + 15) // 16, 2), dtype=torch.float32, device=dev)
            self.pred_logprobs = torch.zeros((max_length, B), dtype=torch.float32, device=dev) if k == 0 else None
        # top-n alternatives: one more launch behind the step end, over the logits and the statistics that one read
        self.pred_top_ids = self.pred_top_logprobs = self.pred_rank = None
        if self.top_logprobs:
            n = self.top_logprobs
            self.pred_top_ids = torch.zeros((max_length, B, n), dtype=torch.int32, device=dev)
            self.pred_top_logprobs = torch.zeros((max_length, B, n), dtype=torch.float32, device=dev)
            self.pred_rank = torch.zeros((max_length, B), dtype=torch.int32, device=dev)
        # truncated sampling: the lm_head call stays the sampling call; the step end finds the cutoff from the logits it stored
        self.top_k, self.top_p, self.min_p = ops.check_truncation(top_k, top_p, min_p)
        self.truncated = self.top_k > 0 or self.top_p < 1.0 or self.min_p > 0.0
        self.pred_cut_y = self.pred_n_kept = None
        if self.truncated:
            if not do_sample:
                raise ValueError("top_k / top_p / min_p truncate the sampler: they need do_sample=True")
            if float(temperature) <= 0.0:
                raise ValueError(f"truncated sampling needs temperature > 0 (got {temperature})")
            need_fused("top_k / top_p / min_p")
        # per-row sampling parameters: the table the lm_head epilogue, the penalty kernel and the step end read
        self.row_table = self.row_params = self.row_streams = None
        if row_sampling is not None:
            need_fused("row_sampling")
            params = list(row_sampling)
            streams = list(range(B)) if row_streams is None else [int(v) for v in row_streams]
            if len(params) != B or len(streams) != B:
                raise ValueError(f"row_sampling / row_streams must hold one entry per sample ({B}), got {len(params)} / {len(streams)}")
            self.row_params, self.row_streams = params, streams
            if k == 0:
                self.row_table = sampling_mod.to_tensor(sampling_mod.pack(params, seed=int(seed), streams=streams), dev)
            else:
                # with drafts the table has one entry per ROW: sample b's k + 1 rows repeat its parameters, seed and stream, and row j
                # draws with the key of the sample's token n_out + j (include/unimedvl_hip.h, speculative decode with sampling); what
                # the pick launch leaves is per row as well
                self.row_table = sampling_mod.to_tensor(sampling_mod.pack(
                    [p for p in params for _ in range(k + 1)], seed=int(seed), streams=[v for v in streams for _ in range(k + 1)],
                    draws=list(range(k + 1)) * B), dev)
                self.row_picks = torch.zeros((R,), dtype=torch.int64, device=dev)
                self.row_logprob = torch.zeros((R,), dtype=torch.float32, device=dev) if self.logprobs else None
                self.row_cut_y = torch.zeros((R,), dtype=torch.float32, device=dev)
                self.row_n_kept = torch.zeros((R,), dtype=torch.int32, device=dev)
        # each step's cutoff value and kept-column count: a truncated step records them, a step with a per-row table always does
        if self.truncated or (self.row_table is not None and k == 0):
            self.pred_cut_y = torch.zeros((max_length, B), dtype=torch.float32, device=dev)
            self.pred_n_kept = torch.zeros((max_length, B), dtype=torch.int32, device=dev)
        w = llm.w
        # K splits of the QKV / o / down GEMMs: "q,o,d" (1 = that GEMM is not split), "0" = none, "auto" by batch / weights.
        # Measured on MI355X (bench.py --batch B, ms per step), no split -> 3,4,4:
        #   B=12: 3.72 -> 3.59, 16: 4.09 -> 3.85, 32: 5.48 -> 4.67, 64: 9.07 -> 6.35; more splits are slower (4,4,8: 4.95 at
        #   B=32); e4m3 weights: x is as many bytes as the weights already at B=8, the split pays there too (2.63 -> 2.52).
        # bf16 at B <= 8 (tools/skinny_bench.py, us per GEMM): QKV 11.4 -> 8.5 with 3 splits, down 25.9 -> 23.3 with 4,
        #   o_proj 8.7 either way (its exact-partition image without a split keeps the residual add in the GEMM).
        sk = os.environ.get("UMV_DECODE_SPLITK", "auto")
        if sk == "auto":
            # (B <= 8 bf16: 3,4,4 3.151 ms vs 3,1,4 3.161 - a wash, so one setting for every batch and weight type; it also
            # makes the exact-partition copy of the o_proj weights unnecessary)
            # 65..128 rows: the same scheme on the 128 x 128 MFMA tile (umv_gemm_bf16 routes k_splits > 1 there above 64 rows):
            # without it down_proj is 14 workgroups of 256 x 256 (151 us); bf16 weights only (the e4m3 image is an M <= 64 layout)
            # MXFP4 weights take both branches: up to 64 rows the split partials of umv_gemm_mxfp4w; 65..128 rows the same K ranges on
            # the tiled MXFP4 kernel (umv_gemm_mxfp4t) when the linears carry no bf16 image of their dequantised weights
            # (llm_fp4_keep_bf16=False), else umv_gemm_bf16 on that image - ops.gemm_splitk routes by rows and by what the linear holds
            sk = "3,4,4" if R <= 64 else ("6,8,8" if R <= 128 and not getattr(w, "fp8", False) else "0")
        self.sk = (1, 1, 1) if sk in ("0", "") else tuple(max(1, int(v)) for v in sk.split(","))
        if len(self.sk) != 3 or any(v > 64 for v in self.sk):
            raise ValueError(f"UMV_DECODE_SPLITK={sk!r}: expected 'q,o,d' with 1 <= splits <= 64")
        if self.sk != (1, 1, 1) and R > 128:
            raise ValueError("split-K decode mode serves at most 128 samples per step")
        sq, so, sd = self.sk
        self.p_qkv = torch.empty((sq, R, (nq + 2 * nkv) * hd), dtype=torch.float32, device=dev) if sq > 1 else None
        self.p_h = torch.empty((max(so, sd), R, H), dtype=torch.float32, device=dev) if max(so, sd) > 1 else None
        # decode-only weight copies with exact-partition tiles (N/256 rows per tile) for the GEMMs that run without a split
        exact = os.environ.get("UMV_DECODE_EXACT_TILES", "1") not in ("0", "") and R <= 64
        need = (sq == 1, so == 1, sd == 1)
        if exact and any(need):
            if not hasattr(w, "decode_copies"):
                w.decode_copies = [[None, None, None] for _ in w.und]
            for lw, slot in zip(w.und, w.decode_copies):
                for i, lin in enumerate((lw.qkv, lw.o, lw.down)):
                    if need[i] and slot[i] is None:
                        slot[i] = lin.for_decode()
            self.dec = [tuple(c if c is not None else lin for c, lin in zip(slot, (lw.qkv, lw.o, lw.down)))
                        for lw, slot in zip(w.und, w.decode_copies)]
        else:
            self.dec = [(lw.qkv, lw.o, lw.down) for lw in w.und]
        # (q/k norm + RoPE + KV append folded into the attention kernel - umv_attn_decode_fused of experimental/ - wins only when the
        # QKV GEMM is not split: B = 8: 3.32 vs 3.39 ms without a split, 3.28 vs 3.24 with the default 3-way split, B = 32: 4.80 vs
        # 4.52; the default path splits, so the step always runs umv_qkv_post + umv_attn_varlen)
        self.do_sample, self.temperature, self.seed = bool(do_sample), float(temperature), int(seed)
        # how the step ends, decided once: what the lm_head call leaves besides the logits, and the call that closes the step
        self.lm_head_kw = {}
        if self.fused_argmax:
            self.lm_head_kw["argmax_partial"] = self.amax_part
            if self.logprobs or self.truncated:
                self.lm_head_kw["lse_partial"] = self.lse_part
            self.lm_head_kw["sample"] = (self.temperature, self.seed, self.step_idx) if self.do_sample else None
            if self.row_table is not None:
                self.lm_head_kw["sample_rows"] = self.row_table
        # what every launch between the lm_head call and the step end is given, so that it rewrites the tiles as that call left them:
        # the temperature as the lm_head call sampled (0 when greedy), its seed and step counter, its keys and statistics, its table
        self.step_kw = dict(temperature=self.temperature if self.do_sample else 0.0, seed=self.seed, step=self.step_idx,
                            argmax_partial=self.lm_head_kw.get("argmax_partial"), lse_partial=self.lm_head_kw.get("lse_partial"),
                            sample_rows=self.row_table)
        # (a name, not a bound method: a session that refers to itself is freed by the cycle collector only - at any allocation, another
        # session's graph capture included, where releasing device memory aborts)
        self.step_end = "rows" if self.row_table is not None else "truncated" if self.truncated else "logprob" if self.logprobs else "argmax" if self.fused_argmax else "unfused"
        # (force: a per-row table holds the penalty values - the scalar ones stay neutral - or reserves the buffers for later rows)
        force = self.row_table is not None and (bool(row_penalties) or any(p.penalised for p in self.row_params))
        self._init_penalties(repetition_penalty, presence_penalty, frequency_penalty, logit_bias, penalty_context_ids,
                             penalty_context_room, penalty_history, force)
        self._init_ngram(no_repeat_ngram_size, ngram_context_ids, ngram_context_room, ngram_history)
        self._init_sequences(bad_words_ids, suppress_tokens, begin_suppress_tokens, min_new_tokens, end_token_id, sequence_row_min)
        self._init_constraint(constraint, constraint_states)
        self.guid = None                            # the tables of classifier-free guidance (guidance.GuidedDecodeSession sets them)
        self.steps_done = 0
        self.graph = None
        if use_graph:
            self._capture()

    # ---- logit penalties (include/unimedvl_hip.h): per slot a count word per column, the list of columns to visit (static entries
    # first: the context and the biased columns, seeded here; then the generated ones, appended by the kernel) and its length
    def _init_penalties(self, repetition_penalty, presence_penalty, frequency_penalty, logit_bias, penalty_context_ids,
                        penalty_context_room, penalty_history, force):
        cfg, dev, B = self.cfg, self.dev, self.B
        r, p, f, bias = ops.check_penalties(repetition_penalty, presence_penalty, frequency_penalty, logit_bias, vocab=cfg.vocab)
        bias = {t: v for t, v in bias.items() if v != 0.0}
        self.pen = None
        self.pen_count = self.pen_list = self.pen_len = self.pen_bias = None
        context = penalty_context_ids
        if r == 1.0 and p == 0.0 and f == 0.0 and not bias and not force:
            return                                  # neutral (a context set alone changes nothing): today's step
        if context is None:
            context = [[] for _ in range(B)]
        if len(context) != B:
            raise ValueError(f"penalty_context_ids must hold one token list per sample ({B}), got {len(context)}")
        context = [self._penalty_context(c) for c in context]
        room = max([len(c) for c in context] + [0]) if penalty_context_room is None else int(penalty_context_room)
        history = self.max_length if penalty_history is None else int(penalty_history)
        self.pen_bias_cols = bias
        self.pen_room = room
        self.pen_static = min(room, cfg.vocab) + len(bias)
        cap = self.pen_static + max(1, min(history, cfg.vocab))
        self.pen = (r, p, f)
        self.pen_count = torch.zeros((B, cfg.vocab), dtype=torch.int32, device=dev)
        self.pen_list = torch.full((B, cap), -1, dtype=torch.int32, device=dev)
        self.pen_len = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self.pen_bias = torch.zeros((B, self.pen_static), dtype=torch.float32, device=dev) if self.pen_static else None
        for b in range(B):
            self._reset_penalty_slot(b, context[b])

    # ---- no-repeat n-grams (include/unimedvl_hip.h): per slot the ordered history - context, start token, then every token fed - and
    # its length; the sizes as one scalar, or one word per slot
    def _init_ngram(self, size, context_ids, context_room, history):
        dev, B = self.dev, self.B
        self.ng_hist = self.ng_len = self.ng_row_n = None
        self.ng_n = 0
        if self.row_params is not None:
            if not (isinstance(size, int) and not isinstance(size, bool) and size == 0):
                raise ValueError(f"row_sampling excludes the scalar no_repeat_ngram_size (got {size!r}): a row's size is its SamplingParams'")
            sizes = [p.no_repeat_ngram_size for p in self.row_params]
            on = any(sizes) or history is not None
        elif isinstance(size, (list, tuple)):
            sizes = [ops.check_ngram(v) for v in size]
            if len(sizes) != B:
                raise ValueError(f"no_repeat_ngram_size must be one integer or one per sample ({B}), got {len(sizes)}")
            on = any(sizes)
        else:
            self.ng_n = ops.check_ngram(size)
            sizes, on = None, self.ng_n > 0
        if not on:
            return                                  # off (a context alone changes nothing): today's step
        if self.draft_len:
            raise ValueError("no_repeat_ngram_size is not available with draft_len > 0 (speculative decode)")
        context = [[] for _ in range(B)] if context_ids is None else [self._ngram_context(c) for c in context_ids]
        if len(context) != B:
            raise ValueError(f"ngram_context_ids must hold one token list per sample ({B}), got {len(context)}")
        room = max([len(c) for c in context] + [0]) if context_room is None else int(context_room)
        history = self.max_length if history is None else int(history)
        if room < 0 or history < 0:
            raise ValueError(f"ngram_context_room / ngram_history must be >= 0 (got {context_room!r} / {history!r})")
        self.ng_room = room
        self.ng_hist = torch.zeros((B, room + max(1, history)), dtype=torch.int32, device=dev)
        self.ng_len = torch.zeros((B,), dtype=torch.int32, device=dev)
        if sizes is not None:
            self.ng_row_n = torch.tensor(sizes, dtype=torch.int32).to(dev)
        for b in range(B):
            self._reset_ngram_slot(b, context[b])

    @staticmethod
    def _ngram_context(tokens):
        """a context list as ints (negative entries are separators), every one an int32"""
        out = [int(t) for t in (tokens.tolist() if hasattr(tokens, "tolist") else tokens or ())]
        if out and (max(out) >= 1 << 31 or min(out) < -(1 << 31)):
            raise ValueError("ngram_context_ids holds a token that is no int32")
        return out

    def _reset_ngram_slot(self, b, context):
        """Slot b starts a request: `context` is its whole history (the step appends the start token)."""
        if len(context) > self.ng_room:
            raise ValueError(f"slot {b}: {len(context)} context tokens, the session reserved room for {self.ng_room} (ngram_context_room)")
        if context:
            self.ng_hist[b, :len(context)] = torch.tensor(context, dtype=torch.int32, device=self.dev)
        self.ng_len[b:b + 1].fill_(len(context))

    @ops.on_device
    def copy_ngram_history(self, other, slots=None):
        """Take over another session's n-gram histories (and per-slot sizes) for `slots` (default: all) - a re-captured step goes on
        with those requests.  This session's rows hold at least what the other's hold."""
        if self.ng_hist is None:
            return
        if other.ng_hist is None or other.ng_hist.shape[0] != self.ng_hist.shape[0] or other.ng_hist.shape[1] > self.ng_hist.shape[1] or \
                (self.ng_row_n is None) != (other.ng_row_n is None):
            raise ValueError("copy_ngram_history: the sessions do not share an n-gram layout")
        rows, at = self._slot_index(slots)
        if not rows:
            return
        hist = torch.zeros((len(rows), self.ng_hist.shape[1]), dtype=torch.int32, device=self.dev)
        hist[:, :other.ng_hist.shape[1]] = other.ng_hist[at]
        self.ng_hist[at] = hist
        self.ng_len[at] = other.ng_len[at]
        if self.ng_row_n is not None:
            self.ng_row_n[at] = other.ng_row_n[at]

    # ---- banned sequences (include/unimedvl_hip.h): one static table for the session; per slot the count of tokens fed, the last 15 of
    # them and, where min_new_tokens is in play, the slot's minimum.  beams (K > 0): the rows are B / K requests of K beams, the kernel
    # takes count and tail from the search's back-pointers (self.seq_beam, set by the beam session) and the session owns no history
    def _init_sequences(self, bad_words_ids, suppress_tokens, begin_suppress_tokens, min_new_tokens, end_token_id, row_entry=False,
                        beams=0):
        dev, B = self.dev, self.B
        self.seq_table = self.seq_tail = self.seq_count = self.seq_row_min = self.seq_beam = None
        requests = B // beams if beams else B
        probe = min_new_tokens.tolist() if hasattr(min_new_tokens, "tolist") else min_new_tokens
        held = any(probe) if isinstance(probe, (list, tuple)) else bool(probe)
        # (an end token that holds nothing back is not looked at)
        _, _, _, mins, end = ops.check_sequences(bad_words_ids, suppress_tokens, begin_suppress_tokens, min_new_tokens,
                                                 end_token_id if held or row_entry else None, vocab=self.cfg.vocab, rows=requests)
        if row_entry and end is None:
            raise ValueError("sequence_row_min reserves the end-token entry: it needs end_token_id")
        ptr, tok, until, _ = ops.sequence_table(bad_words_ids, suppress_tokens, begin_suppress_tokens, mins, end, vocab=self.cfg.vocab,
                                                row_entry=row_entry)
        if not len(until):
            return                                  # off: today's step
        if self.draft_len:
            raise ValueError("bad_words_ids / suppress_tokens / begin_suppress_tokens / min_new_tokens are not available with "
                             "draft_len > 0 (speculative decode)")
        self.seq_table = ops.SequenceTable(ptr, tok, until, dev)
        if int(until[-1]) == ops.SEQ_ROW:
            per = mins if isinstance(mins, list) else [mins] * requests
            self.seq_row_min = torch.tensor([n for n in per for _ in range(max(1, beams))], dtype=torch.int32).to(dev)
        if not beams:
            self.seq_tail = torch.full((B, ops.SEQ_TAIL), -1, dtype=torch.int32, device=dev)
            self.seq_count = torch.zeros((B,), dtype=torch.int32, device=dev)

    def _reset_sequence_slot(self, b, min_new_tokens=None):
        """Slot b starts a request: nothing fed yet; min_new_tokens (None: as it is) becomes the slot's minimum."""
        if min_new_tokens is not None:
            n = ops.check_sequences(min_new_tokens=min_new_tokens, end_token_id=0)[3]
            if isinstance(n, list):
                raise ValueError(f"set_slot(min_new_tokens=...) takes one integer, got {min_new_tokens!r}")
            if self.seq_row_min is None:
                if n:
                    raise ValueError("this session reserved no minimums: build it with min_new_tokens or sequence_row_min=True (and end_token_id)")
            else:
                self.seq_row_min[b:b + 1].fill_(n)
        if self.seq_tail is not None:
            self.seq_tail[b].fill_(-1)
            self.seq_count[b:b + 1].fill_(0)

    @ops.on_device
    def copy_sequence_state(self, other, slots=None):
        """Take over another session's banned-sequence state (counts, tails, minimums) for `slots` (default: all) - a re-captured step
        goes on with those requests.  The sessions were built with the same table; one that carried no minimums leaves this one's as
        they were built."""
        if self.seq_tail is None or other.seq_tail is None:      # (a session that had no table had nothing banned: nothing to take)
            return
        if other.seq_tail.shape != self.seq_tail.shape:
            raise ValueError("copy_sequence_state: the sessions do not hold the same slots")
        rows, at = self._slot_index(slots)
        if not rows:
            return
        self.seq_tail[at] = other.seq_tail[at]
        self.seq_count[at] = other.seq_count[at]
        if self.seq_row_min is not None and other.seq_row_min is not None:
            self.seq_row_min[at] = other.seq_row_min[at]

    # ---- constrained decoding (include/unimedvl_hip.h, token automata): the automaton's tables and one state word per sample
    def _init_constraint(self, automaton, states):
        self.constraint = self.con_dev = self.con_state = None
        if automaton is None:
            return
        from .constraints import TokenAutomaton
        if not isinstance(automaton, TokenAutomaton):
            raise ValueError(f"constraint must be a constraints.TokenAutomaton, got {type(automaton).__name__}")
        states = [0] * self.B if states is None else [self._constraint_state(automaton, s) for s in states]
        if len(states) != self.B:
            raise ValueError(f"constraint_states must hold one start state per sample ({self.B}), got {len(states)}")
        self.constraint = automaton
        self.con_dev = automaton.to_device(self.dev)
        self.con_state = torch.tensor(states, dtype=torch.int32).to(self.dev)

    @staticmethod
    def _constraint_state(automaton, s):
        if isinstance(s, bool) or int(s) != s or not -1 <= int(s) < automaton.n_states:
            raise ValueError(f"a constraint state must be an integer in [-1, {automaton.n_states}) (-1 = unconstrained), got {s!r}")
        return int(s)

    @ops.on_device
    def copy_constraint_states(self, other, slots=None):
        """Take over another session's state words for `slots` (default: all) - a re-captured step goes on with those requests.  The
        sessions were built with the same automaton."""
        if self.con_state is None:
            return
        if other.con_state is None or other.constraint is not self.constraint:
            raise ValueError("copy_constraint_states: the sessions do not share an automaton")
        rows, at = self._slot_index(slots)
        if rows:
            self.con_state[at] = other.con_state[at]

    def _slot_index(self, slots):
        """`slots` (default: all) as a list and as an index tensor on the device"""
        rows = list(range(self.B)) if slots is None else [int(b) for b in slots]
        return rows, torch.tensor(rows, dtype=torch.int64, device=self.dev)

    def _penalty_context(self, tokens):
        """distinct tokens of a context list, in order of first appearance"""
        out = list(dict.fromkeys(int(t) for t in (tokens.tolist() if hasattr(tokens, "tolist") else tokens or ())))
        if any(t < 0 or t >= self.cfg.vocab for t in out):
            raise ValueError(f"penalty_context_ids holds a token outside [0, {self.cfg.vocab})")
        return out

    def _reset_penalty_slot(self, b, context):
        """Slot b starts a request: no generated tokens, `context` (distinct tokens) as its context set, the length word "fresh"."""
        if len(context) > self.pen_room:
            raise ValueError(f"slot {b}: {len(context)} distinct context tokens, the session reserved room for {self.pen_room} "
                             "(penalty_context_room)")
        listed, ctx = _lib_flag(_lib.PENALTY_LISTED), _lib_flag(_lib.PENALTY_LISTED | _lib.PENALTY_CONTEXT)
        inside = set(context)
        cols = context + [t for t in self.pen_bias_cols if t not in inside]
        words = [ctx] * len(context) + [listed] * (len(cols) - len(context))
        self.pen_count[b].zero_()
        self.pen_list[b, :self.pen_static].fill_(-1)
        if cols:
            at = torch.tensor(cols, dtype=torch.int64, device=self.dev)
            self.pen_count[b, at] = torch.tensor(words, dtype=torch.int32, device=self.dev)
            self.pen_list[b, :len(cols)] = at.to(torch.int32)
            self.pen_bias[b].zero_()
            self.pen_bias[b, :len(cols)] = torch.tensor([self.pen_bias_cols.get(t, 0.0) for t in cols], dtype=torch.float32, device=self.dev)
        self.pen_len[b:b + 1].fill_(-1)

    @ops.on_device
    def copy_penalty_history(self, other, slots=None):
        """Take over another session's penalty state for `slots` (default: all) - a re-captured step goes on with those requests.  The
        sessions hold the same slots and biased columns; this one's static section and list may be larger (more room for context)."""
        if self.row_table is not None:              # the kept slots go on with their parameters, streams and draw counters
            if other.row_table is None:
                raise ValueError("copy_penalty_history: the other session has no per-row sampling table")
            keep, at = self._slot_index(slots)
            if keep:
                self.row_table[at] = other.row_table[at]
                for b in keep:
                    self.row_params[b], self.row_streams[b] = other.row_params[b], other.row_streams[b]
        if self.pen is None:
            return
        grow = 0 if other.pen is None else self.pen_static - other.pen_static
        if other.pen is None or other.pen_count.shape != self.pen_count.shape or other.pen_bias_cols != self.pen_bias_cols or grow < 0 or \
                other.pen_list.shape[1] + grow > self.pen_list.shape[1]:
            raise ValueError("copy_penalty_history: the sessions do not share a penalty layout")
        rows, at = self._slot_index(slots)
        if not rows:
            return
        old, n_gen = other.pen_static, other.pen_list.shape[1] - other.pen_static
        self.pen_count[at] = other.pen_count[at]
        lst = torch.full((len(rows), self.pen_list.shape[1]), -1, dtype=torch.int32, device=self.dev)
        lst[:, :old] = other.pen_list[at, :old]                                          # static entries, then this session's extra room
        lst[:, self.pen_static:self.pen_static + n_gen] = other.pen_list[at, old:]       # the generated columns follow the static section
        self.pen_list[at] = lst
        ln = other.pen_len[at]
        self.pen_len[at] = torch.where(ln < 0, ln, ln + grow)
        if self.pen_bias is not None:
            bias = torch.zeros((len(rows), self.pen_static), dtype=torch.float32, device=self.dev)
            if old:
                bias[:, :old] = other.pen_bias[at]
            self.pen_bias[at] = bias

    def _step(self):
        cfg, w, c = self.cfg, self.llm.w, self.cache
        nq, nkv, hd = cfg.heads, cfg.kv_heads, cfg.head_dim
        L = cfg.layers
        sq, so, sd = self.sk
        ops.embed_gather(w.embed, self.ids, out=self.seq)      # in_ids[step] already holds these tokens (decode_step_end)
        ops.rmsnorm(self.seq, w.und[0].in_norm, cfg.rms_eps, out=self.x)
        for l in range(L):
            lw = w.und[l]
            qkv_w, o_w, down_w = self.dec[l]
            # ---- attention block: QKV (bias in the GEMM epilogue, or added by the consumer of the partial sums)
            if sq > 1:
                ops.gemm_splitk(self.x, lw.qkv, self.p_qkv, sq)
                part = dict(partials=self.p_qkv, bias=lw.qkv.bias)
            else:
                ops.gemm(self.x, qkv_w, out=self.qkv)
                part = {}
            ops.qkv_post(None if part else self.qkv, self.q, c.slabs[l], self.tok_seg, self.tok_slot, self.tok_pos, nq, nkv, hd,
                         cfg.rms_eps, lw.q_norm, lw.k_norm, cos_tab=w.cos, sin_tab=w.sin, **part)
            ops.attention(self.q, self.o, c.slabs[l], self.cu_q, self.kv_len, nq, nkv, hd, True, self.draft_len + 1, self.max_kv,
                          self.nsplit, self.ws, wave_split=self.wave_split)
            # ---- o_proj + residual, then the post-attention norm
            if so > 1:
                ops.gemm_splitk(self.o, lw.o, self.p_h[:so], so)
                ops.residual_rmsnorm(self.p_h[:so], self.seq, lw.post_norm, cfg.rms_eps, out=self.x)
            else:
                ops.gemm(self.o, o_w, out=self.seq, residual=self.seq)
                ops.rmsnorm(self.seq, lw.post_norm, cfg.rms_eps, out=self.x)
            # ---- MLP: SwiGLU in the gate/up epilogue, down + residual, then the NEXT layer's input norm (or the final norm)
            ops.gemm(self.x, lw.gate_up, out=self.act)
            last = l + 1 == L
            nxt, dst = (w.norm, self.hn) if last else (w.und[l + 1].in_norm, self.x)
            if sd > 1:
                ops.gemm_splitk(self.act, lw.down, self.p_h[:sd], sd)
                ops.residual_rmsnorm(self.p_h[:sd], self.seq, nxt, cfg.rms_eps, out=dst)
            else:
                ops.gemm(self.act, down_w, out=self.seq, residual=self.seq)
                ops.rmsnorm(self.seq, nxt, cfg.rms_eps, out=dst)
        ops.gemm(self.hn, w.lm_head, out=self.logits, **self.lm_head_kw)
        if self.guid is not None:
            # first behind the lm_head call (HF's processor order): every guided row becomes the contrast of its log-softmax with its
            # unconditional row's, its tiles' keys and statistics rewritten with what the lm_head call got
            ops.logit_guidance(self.logits, temperature=self.step_kw["temperature"], seed=self.seed, step=self.step_idx,
                               argmax_partial=self.amax_part, lse_partial=self.lse_part, **self.guid)
        if self.pen is not None:
            # record the token this step was fed, patch the logits of the seen / biased columns, recompute the tiles they sit in - with
            # the (temperature, seed, step) the lm_head call got, so whichever step end follows reads the adjusted distribution
            r, p, f = self.pen
            ops.logit_penalty(self.logits, self.ids, self.pen_count, self.pen_list, self.pen_len, self.pen_static, bias=self.pen_bias,
                              repetition_penalty=r, presence_penalty=p, frequency_penalty=f, **self.step_kw)
        if self.ng_hist is not None:
            # record the token this step is fed in every sample's history and set the columns that would repeat an n-gram of it to
            # -inf, their tiles' keys and statistics with them - again with what the lm_head call got
            ops.logit_ngram_ban(self.logits, self.ids, self.ng_hist, self.ng_len, n=self.ng_n, row_n=self.ng_row_n, **self.step_kw)
        if self.seq_table is not None:
            # record the token this step is fed in every sample's count and tail (a beam search: read them off its back-pointers) and set
            # the columns the table bans to -inf, their tiles' keys and statistics with them - again with what the lm_head call got
            ops.logit_sequence_ban(self.logits, self.ids, self.seq_table, tail=self.seq_tail, count=self.seq_count,
                                   row_min=self.seq_row_min, beam=self.seq_beam, **self.step_kw)
        if self.con_state is not None:
            # mask the (adjusted) logits of every constrained sample to its state's tokens and rewrite its tiles' keys and statistics,
            # again with what the lm_head call got: the step end picks from, and normalises over, the allowed set
            ops.logit_constrain(self.logits, self.con_dev, self.con_state, **self.step_kw)
        self._step_end()
        if self.guid is not None:
            ops.guidance_feed(self.guid["pair"], self.ids, self.in_ids, self.pred_ids, self.step_idx)   # the pick of a guided row is its partner's too
        if self.top_logprobs:
            # the n best columns of the (adjusted) logits and the rank of the token just fed, with the statistics merged as the step end did
            ops.decode_top_logprobs(self.logits, self.lse_part, self.ids, self.step_idx, self.pred_top_ids, self.pred_top_logprobs,
                                    self.pred_rank, temperature=self.step_kw["temperature"], sample_rows=self.step_kw["sample_rows"],
                                    truncated=self.step_end == "truncated", forced_ids=self.forced_ids)
        if self.con_state is not None:
            ops.constraint_advance(self.con_dev, self.con_state, self.ids)     # along the token the next step is fed: picked or forced

    def _step_end(self):
        """the launch that closes the step: the pick (where the lm_head epilogue left keys) and the bookkeeping"""
        if self.step_end == "rows":
            # every row ends the step with its own sampler (the truncated path or the key maximum) and advances its own draw counter
            ops.decode_step_end_rows(self.tok_slot, self.tok_pos, self.kv_len, self.amax_part, self.ids, self.in_ids, self.pred_ids,
                                     self.step_idx, self.logits, self.row_table, lse_partial=self.lse_part, logprobs=self.pred_logprobs,
                                     forced_ids=self.forced_ids, cut_y=self.pred_cut_y, n_kept=self.pred_n_kept)
        elif self.step_end == "truncated":
            # the fused step end whose pick is the epilogue's only if that column survived the filters (the kept set's Gumbel maximum
            # otherwise), plus pred_cut_y[step] / pred_n_kept[step] - and pred_logprobs[step] when log-probabilities are on
            ops.decode_step_end_truncated(self.tok_slot, self.tok_pos, self.kv_len, self.amax_part, self.ids, self.in_ids, self.pred_ids,
                                          self.step_idx, self.logits, self.temperature, self.seed, self.top_k, self.top_p, self.min_p,
                                          lse_partial=self.lse_part, logprobs=self.pred_logprobs, forced_ids=self.forced_ids,
                                          cut_y=self.pred_cut_y, n_kept=self.pred_n_kept)
        elif self.step_end == "logprob":
            # the fused step end below, plus pred_logprobs[step] = log-probability of the token fed next (the pick or the forced one)
            ops.decode_step_end_logprob(self.tok_slot, self.tok_pos, self.kv_len, self.amax_part, self.lse_part, self.ids, self.in_ids,
                                        self.pred_ids, self.step_idx, self.logits, self.pred_logprobs,
                                        self.temperature if self.do_sample else 0.0, self.forced_ids)
        elif self.step_end == "argmax":
            # ids = argmax; pred_ids[step] = in_ids[step + 1] = ids; slot / position / kv_len / step += 1: one launch
            ops.decode_step_end_argmax(self.tok_slot, self.tok_pos, self.kv_len, self.amax_part, self.ids, self.in_ids, self.pred_ids,
                                       self.step_idx)
        else:
            if self.do_sample:
                ops.sample(self.logits, self.temperature, self.seed, step=self.step_idx, out=self.ids)
            else:
                ops.argmax(self.logits, out=self.ids)
            # pred_ids[step] = in_ids[step + 1] = ids; slot / position / kv_len / step += 1: one launch
            ops.decode_step_end(self.tok_slot, self.tok_pos, self.kv_len, self.ids, self.in_ids, self.pred_ids, self.step_idx)

    def _state(self):
        """every tensor a step writes that the next one reads"""
        state = (self.ids, self.tok_slot, self.tok_pos, self.kv_len, self.step_idx)
        if self.pen is not None:                    # a step records into the penalty history as well
            state += (self.pen_count, self.pen_list, self.pen_len)
        if self.row_table is not None:              # ... and advances the rows' draw counters
            state += (self.row_table,)
        if self.con_state is not None:              # ... and the constraint states
            state += (self.con_state,)
        if self.ng_hist is not None:                # ... and appends to the n-gram histories
            state += (self.ng_hist, self.ng_len)
        if self.seq_tail is not None:               # ... and records in the banned-sequence counts and tails
            state += (self.seq_tail, self.seq_count)
        return state

    def _capture(self):
        # the captured step appends at slot = lens0 and bumps the counters; warm up on a side
        # stream first (lazy module loading), then restore the counters so capture sees a clean state
        state = self._state()
        saved = [t.clone() for t in state]
        s = torch.cuda.Stream(device=self.dev)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        for t, v in zip(state, saved):
            t.copy_(v)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step()
        # capture does not execute; counters are still at their initial values
        self.graph = g

    @ops.on_device
    def step(self, n=1):
        for _ in range(n):
            if self.steps_done >= self.max_length:
                raise RuntimeError("decode session exhausted")
            if self.graph is not None:
                self.graph.replay()
            else:
                self._step()
            self.steps_done += 1

    # ---- continuous batching support (serving.py): the captured step reads these from device memory, so a slot can be
    # re-pointed at a new request between replays without re-capturing
    @ops.on_device
    def set_slot(self, b, token, kv_len, pos, penalty_context_ids=None, sampling=None, stream=None, draw=0, constraint_state=None,
                 ngram_context_ids=None, min_new_tokens=None):
        """Sample b continues from `token` with `kv_len` tokens already in its cache segment and rope position `pos`.  With penalties
        on, the slot's history starts over: no generated tokens, penalty_context_ids as its context set, `token` as its start token.
        sampling (a SamplingParams; sessions with row_sampling): row b of the table is rewritten - the slot decodes with these
        parameters from the next replay on, its key words (seed, stream - default: the slot's current one -, draw); without it the
        row, its draw counter included, stays as it is.
        constraint_state (sessions with constraint): the slot's state word becomes this state of the automaton (-1 = unconstrained)
        from the next replay on; without it the word stays as it is.
        With no_repeat_ngram_size on, the slot's n-gram history starts over as well: ngram_context_ids (default: nothing) is what
        precedes `token` in it; with row_sampling, `sampling` also brings the slot's size.
        With banned sequences on, the slot's count and tail start over too; min_new_tokens (sessions built with min_new_tokens or
        sequence_row_min) becomes the slot's own minimum, without it the minimum stays as it is."""
        if constraint_state is not None:
            if self.con_state is None:
                raise ValueError("set_slot(constraint_state=...) needs a session built with constraint")
            self.con_state[b:b + 1].fill_(self._constraint_state(self.constraint, constraint_state))
        if sampling is not None:
            self._set_row(b, sampling, stream, draw)
        if self.pen is not None:
            self._reset_penalty_slot(b, self._penalty_context(penalty_context_ids))
        if self.ng_hist is not None:
            self._reset_ngram_slot(b, self._ngram_context(ngram_context_ids))
        if self.seq_table is not None or min_new_tokens is not None:
            self._reset_sequence_slot(b, min_new_tokens)
        self.ids[b:b + 1].fill_(int(token))
        self.tok_slot[b:b + 1].fill_(int(kv_len))
        self.kv_len[b:b + 1].fill_(int(kv_len) + 1)
        self.tok_pos[b:b + 1].fill_(int(pos))

    def _set_row(self, b, params, stream, draw):
        if self.row_table is None:
            raise ValueError("set_slot(sampling=...) needs a session built with row_sampling")
        if self.pen is None and params.penalised:
            raise ValueError("this session reserved no penalty buffers: build it with row_penalties=True (or a penalised row)")
        if params.no_repeat_ngram_size and self.ng_hist is None:
            raise ValueError("this session reserved no n-gram history: build it with ngram_history= (or a row with a size)")
        if self.ng_row_n is not None:
            self.ng_row_n[b:b + 1].fill_(params.no_repeat_ngram_size)
        stream = self.row_streams[b] if stream is None else int(stream)
        row = sampling_mod.to_tensor(sampling_mod.pack_row(params, seed=self.seed, stream=stream, draw=draw), self.dev)
        self.row_table[b:b + 1].copy_(row)
        self.row_params[b], self.row_streams[b] = params, stream

    @ops.on_device
    def rewind_outputs(self):
        """Start writing in_ids / pred_ids (and pred_logprobs) at row 0 again (the caller has harvested the previous rows).  The
        penalty history is NOT touched: a request lives across rounds - and neither are the rows' draw counters (row_sampling): a
        request's noise does not repeat from round to round - nor the constraint states: a request is where it is in its automaton -
        nor the n-gram histories, nor the banned-sequence counts, tails and minimums."""
        self.step_idx.zero_()
        self.in_ids[0].copy_(self.ids)      # the tokens the next step is fed (set_slot may have changed them)
        self.steps_done = 0

    def commit(self, steps=None):
        """Make the cache's host-side lengths reflect `steps` decoded tokens."""
        steps = self.steps_done if steps is None else steps
        self.cache.lens = [l + steps for l in self.lens0]
