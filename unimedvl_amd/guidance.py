"""Classifier-free guidance for text (include/unimedvl_hip.h, "classifier-free guidance for text").

B requests decode as R = 2 B ordinary rows of the decode step: rows 0 .. B - 1 over the conditional contexts, rows B .. 2 B - 1 over
their unconditional partners (the same prompt without its images, or a negative prompt) - every row its own segment of one cache,
through DecodeSession's layer loop, one copy of it.  Behind the lm_head call one stage rewrites every conditional row to
g * (log_softmax(cond) - log_softmax(uncond)) + log_softmax(uncond) and its tiles' keys and statistics with it, the ordinary step end
picks, and one small launch behind it hands each pick to the partner row: both rows are fed the same token.  One HIP graph per step.
"""
import math

import torch

from . import ops
from .decode import DecodeSession


class GuidedDecodeSession(DecodeSession):
    """A DecodeSession over `cache`, whose 2 B segments are the B conditional contexts followed by their B unconditional partners.
    start_tokens: one per request (both rows of a pair start from it).  positions / guidance_positions: the rope positions of the
    conditional / unconditional rows, one per request each.  guidance_scale (finite, >= 0; a float, or one per request) and
    guidance_plausibility (beta in [0, 1); a float, or one per request): HF's guidance_scale and the plausibility floor of contrastive
    decoding.  The pair, scale and floor tables live in device memory (self.guid).  Combines with greedy decoding, do_sample /
    temperature, top_k / top_p / min_p, logprobs and top_logprobs - all defined on the guided logits; everything else DecodeSession
    takes is refused (ops.GUIDANCE_EXCLUDES).  The accessors - tokens(), fed(), token_logprobs(), top() - return the conditional rows only;
    in_ids / pred_ids and the other per-row buffers hold all 2 B rows."""

    def __init__(self, llm, cache, start_tokens, positions, max_length, guidance_scale, *, guidance_positions, guidance_plausibility=0.0,
                 use_graph=True, nsplit=None, do_sample=False, temperature=1.0, seed=0, logprobs=False, top_logprobs=0, top_k=0, top_p=1.0,
                 min_p=0.0, **excluded):
        R = len(cache.lens)
        if R % 2 or R > 64 or R == 0:
            raise ValueError(f"a guided session runs over 2 B <= 64 segments (B conditional contexts, then their B unconditional "
                             f"partners), got {R}")
        if hasattr(cache, "ensure_tokens"):
            raise ValueError("guidance_scale decodes on slab caches (NaiveCache): a PagedCache is not available")
        B = R // 2
        scales = list(guidance_scale) if isinstance(guidance_scale, (list, tuple)) else [guidance_scale] * B
        betas = list(guidance_plausibility) if isinstance(guidance_plausibility, (list, tuple)) else [guidance_plausibility] * B
        if len(scales) != B or len(betas) != B:
            raise ValueError(f"guidance_scale / guidance_plausibility: one value, or one per request ({B})")
        checked = [ops.check_guidance(g, b if float(g) != 1.0 else 0.0, **excluded) for g, b in zip(scales, betas)]
        if all(g == 1.0 for g, _ in checked):       # (then nothing above looked at the other keywords)
            ops.check_guidance(2.0, 0.0, **excluded)
        top_logprobs = ops.check_top_logprobs(top_logprobs, llm.cfg.vocab)
        self.requests = B
        self.want_logprobs = bool(logprobs) or top_logprobs > 0
        with ops.device_scope(llm.device):
            starts = torch.as_tensor(start_tokens).reshape(-1)
            pos = torch.cat([torch.as_tensor(positions).reshape(-1).cpu(), torch.as_tensor(guidance_positions).reshape(-1).cpu()])
            if starts.numel() != B or pos.numel() != R:
                raise ValueError(f"start_tokens, positions and guidance_positions hold one entry per request ({B})")
            # always with statistics: the stage reads the rows' log-sum-exp off them
            self._init(llm, cache, starts.repeat(2), pos, max_length, use_graph=False, nsplit=nsplit, do_sample=do_sample,
                       temperature=temperature, seed=seed, logprobs=True, top_logprobs=top_logprobs, top_k=top_k, top_p=top_p, min_p=min_p)
            if not self.fused_argmax:
                raise ValueError("guidance_scale != 1 rides on the fused step end: UMV_DECODE_FUSED_ARGMAX must not be 0")
            dev, f32 = self.dev, torch.float32
            pair = ops.check_guidance_pairs(list(range(B, R)) + [-1] * B, R)
            reuse = self.step_kw["temperature"] in (0.0, 1.0)      # the lm_head call's own statistics are the temperature-0 tile pairs
            self.guid = dict(
                pair=torch.tensor(pair, dtype=torch.int32).to(dev),
                scale=torch.tensor([g for g, _ in checked] + [1.0] * B, dtype=f32).to(dev),
                log_beta=torch.tensor([math.log(b) if b > 0.0 else -math.inf for _, b in checked] + [-math.inf] * B, dtype=f32).to(dev),
                lse=torch.zeros((R,), dtype=f32, device=dev), row_max=torch.zeros((R,), dtype=f32, device=dev),
                stats=None if reuse else torch.zeros_like(self.lse_part))
            if use_graph:
                self._capture()

    @property
    def lse(self):
        """the log-sum-exp words of the last step's rows, fp32 [2 B] (the stage's output)"""
        return self.guid["lse"]

    def fed(self, rows=None):
        """in_ids of the conditional rows: [rows, B], row 0 the start tokens"""
        return self.in_ids[:rows, :self.requests]

    def tokens(self, rows=None):
        """pred_ids of the conditional rows: [rows, B]"""
        return self.pred_ids[:rows, :self.requests]

    def token_logprobs(self, rows=None):
        """pred_logprobs of the conditional rows - those of the guided distribution: [rows, B]"""
        return self.pred_logprobs[:rows, :self.requests]

    def top(self, rows=None):
        """(pred_top_ids, pred_top_logprobs, pred_rank) of the conditional rows"""
        B = self.requests
        return self.pred_top_ids[:rows, :B], self.pred_top_logprobs[:rows, :B], self.pred_rank[:rows, :B]

    def set_slot(self, *a, **kw):
        raise RuntimeError("a guided session's rows are paired: set_slot is not available (the batcher is DESIGN.md section 7)")
