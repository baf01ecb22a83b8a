"""Per-request sampling parameters: SamplingParams and the per-row table the decode step reads (include/unimedvl_hip.h,
umv_row_sampling).

One captured decode step serves rows with different samplers: the lm_head epilogue, the penalty kernel and umv_decode_step_end_rows take
a row's temperature, filters, penalties and the three words of its sampling key - (seed, draw, stream) - from one 48-byte entry per row
in device memory.  This module validates the values on the host (a C entry cannot look into device memory) and packs them."""
from dataclasses import dataclass, fields
from typing import Optional

import numpy as np

from . import ops

# umv_row_sampling, field for field (tests/test_row_sampling_cpu.py holds the offsets to the header with the host compiler)
ROW_DTYPE = np.dtype({
    "names": ["seed", "draw", "stream", "temperature", "top_k", "top_p", "min_p", "repetition_penalty", "presence_penalty",
              "frequency_penalty"],
    "formats": [np.uint64, np.int64, np.uint32, np.float32, np.int32, np.float32, np.float32, np.float32, np.float32, np.float32],
    "offsets": [0, 8, 16, 20, 24, 28, 32, 36, 40, 44],
    "itemsize": 48,
})
ROW_WORDS = ROW_DTYPE.itemsize // 8           # the table as an int64 [B, 6] tensor: column 1 is `draw`
_MASK64 = (1 << 64) - 1


@dataclass(frozen=True)
class SamplingParams:
    """How one request picks its tokens.  do_sample=False: greedy (temperature and the filters must then be at their defaults - a
    filter without a sampler is an error, not a silent no-op).  The penalties apply to greedy and sampled requests alike.
    seed: the request's own seed; None = derived by whoever admits the request (DecodeSession: the session's seed; ContinuousBatcher:
    from the batcher's seed and the request id)."""
    do_sample: bool = False
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    min_p: float = 0.0
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    seed: Optional[int] = None
    no_repeat_ngram_size: int = 0       # (include/unimedvl_hip.h, no-repeat n-grams; 0 = off) - not part of the packed table: the
                                        # sizes travel in an int32 array of their own

    def __post_init__(self):
        if not isinstance(self.do_sample, (bool, np.bool_)):
            raise ValueError(f"do_sample must be a bool, got {self.do_sample!r}")
        t = self.temperature
        if isinstance(t, bool) or not isinstance(t, (int, float)) or t != t or t in (float("inf"), float("-inf")):
            raise ValueError(f"temperature must be a finite number, got {t!r}")
        k, p, m = ops.check_truncation(self.top_k, self.top_p, self.min_p)
        r, pr, fr, _ = ops.check_penalties(self.repetition_penalty, self.presence_penalty, self.frequency_penalty)
        if self.do_sample and not float(t) > 0.0:
            raise ValueError(f"do_sample needs temperature > 0 (got {t!r})")
        if not self.do_sample and (k > 0 or p < 1.0 or m > 0.0):
            raise ValueError("top_k / top_p / min_p truncate the sampler: they need do_sample=True")
        if self.seed is not None and (isinstance(self.seed, bool) or not isinstance(self.seed, int)):
            raise ValueError(f"seed must be an integer or None, got {self.seed!r}")
        object.__setattr__(self, "no_repeat_ngram_size", ops.check_ngram(self.no_repeat_ngram_size))
        for name, v in (("temperature", float(t)), ("top_k", k), ("top_p", p), ("min_p", m), ("repetition_penalty", r),
                        ("presence_penalty", pr), ("frequency_penalty", fr)):
            object.__setattr__(self, name, v)

    @property
    def truncated(self):
        return self.do_sample and (self.top_k > 0 or self.top_p < 1.0 or self.min_p > 0.0)

    @property
    def penalised(self):
        return self.repetition_penalty != 1.0 or self.presence_penalty != 0.0 or self.frequency_penalty != 0.0


# the scalar sampler keywords of DecodeSession, Bagel.generate_text and ContinuousBatcher: SamplingParams' own fields but the seed and the n-gram size (a keyword of its own)
_NEUTRAL = {f.name: f.default for f in fields(SamplingParams) if f.name not in ("seed", "no_repeat_ngram_size")}


def off_neutral(given):
    """The scalar sampler keywords that `given` (a mapping holding every one of them, e.g. a function's locals()) has off its neutral
    value - SamplingParams' default; for do_sample anything but False - in field order"""
    return [k for k, neutral in _NEUTRAL.items() if (given[k] is not False if k == "do_sample" else given[k] != neutral)]


def per_sample(sampling, B):
    """one SamplingParams for all, or a sequence of one per sample -> a list of B SamplingParams"""
    params = [sampling] * B if isinstance(sampling, SamplingParams) else list(sampling)
    if len(params) != B or any(not isinstance(p, SamplingParams) for p in params):
        raise ValueError(f"sampling must be one SamplingParams or a list of one per sample ({B})")
    return params


def from_keywords(do_sample=False, temperature=1.0, **rest):
    """The SamplingParams that the scalar sampler keywords describe (a temperature means nothing without do_sample); ValueError as
    SamplingParams raises it - a filter without do_sample among them"""
    return SamplingParams(do_sample=bool(do_sample), temperature=temperature if do_sample else 1.0, **rest)


def derive_seed(base, rid):
    """The seed of request `rid` under a batcher seeded with `base`: splitmix64 of the two words, on the host - a function of the
    request alone, whatever slot or round it is served in."""
    x = ((int(base) & _MASK64) ^ ((int(rid) + 1) * 0xD1B54A32D192ED03)) & _MASK64
    x = (x + 0x9E3779B97F4A7C15) & _MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _MASK64
    return x ^ (x >> 31)


def pack_row(p, seed=0, stream=0, draw=0):
    """One table entry (a ROW_DTYPE scalar array of shape [1]).  seed: used when the params carry none.  do_sample=False packs
    temperature 0 - the kernels' greedy mark - and neutral filters."""
    if not isinstance(p, SamplingParams):
        raise ValueError(f"expected SamplingParams, got {type(p).__name__}")
    if int(draw) < 0 or not 0 <= int(stream) < (1 << 32):
        raise ValueError(f"draw must be >= 0 and stream a 32-bit unsigned word (got draw={draw!r}, stream={stream!r})")
    row = np.zeros(1, dtype=ROW_DTYPE)
    row["seed"] = np.uint64((p.seed if p.seed is not None else int(seed)) & _MASK64)
    row["draw"], row["stream"] = int(draw), int(stream)
    row["temperature"] = p.temperature if p.do_sample else 0.0
    row["top_k"], row["top_p"], row["min_p"] = (p.top_k, p.top_p, p.min_p) if p.do_sample else (0, 1.0, 0.0)
    row["repetition_penalty"], row["presence_penalty"], row["frequency_penalty"] = p.repetition_penalty, p.presence_penalty, \
        p.frequency_penalty
    return row


def pack(params, seed=0, streams=None, draws=None):
    """The table of a list of SamplingParams: a ROW_DTYPE array [B].  streams (default: all 0) / draws (default: all 0): per row."""
    params = list(params)
    streams = [0] * len(params) if streams is None else list(streams)
    draws = [0] * len(params) if draws is None else list(draws)
    if len(streams) != len(params) or len(draws) != len(params):
        raise ValueError("streams / draws must hold one entry per row")
    if not params:
        return np.zeros(0, dtype=ROW_DTYPE)
    return np.concatenate([pack_row(p, seed, s, d) for p, s, d in zip(params, streams, draws)])


def to_tensor(table, device):
    """The packed table on `device` as an int64 [B, 6] tensor (16-byte aligned: a fresh allocation)."""
    import torch
    words = np.ascontiguousarray(table).view(np.int64).reshape(-1, ROW_WORDS)
    return torch.from_numpy(words.copy()).to(device)


def from_tensor(t):
    """The table back on the host as a ROW_DTYPE array [B]"""
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(ROW_DTYPE).reshape(-1)
