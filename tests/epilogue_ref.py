"""Explicit reference model of the GEMM epilogues (csrc/gemm_epilogue.h) on CPU tensors, for value-exhaustive tests.

One fp64 operation per kernel step on bf16 / fp32 operands, rounded fp64 -> fp32 -> bf16 (vae_ref.rbf) exactly where epi_store4 /
epi_swiglu4 round - and therefore where every other copy of the epilogue (epi_wave_tile_lds, epi_wave_tile_lean<KIND>, their SwiGLU
forms) must round too:
    pre     = rbf(acc + bias)
    act     = rbf(gelu(pre)) | rbf(silu(pre))
    out     = rbf(pre_or_act + residual)
    swiglu  = rbf(rbf(silu(rbf(g))) * rbf(u))
    OUT_F32 = fp32(acc + bias)
A single fp32 + or * of two fp32 values is exact in fp64 (53 >= 2 * 24 + 2), so each add / multiply step equals the kernel's bit for
bit.  The two activations are not exact on the device (v_exp_f32 / v_rcp_f32, about 1 fp32 ulp each, results below 2^-126 flushed):
the model holds their IDEAL values and check_act() states how far a kernel may be from them.

The ideal functions are written free of cancellation:
    silu(x) = x / (1 + exp(-x))
    gelu(x) = x / (1 + exp(-2 u)),  u = sqrt(2 / pi) * (x + 0.044715 x^3)       (torch's approximate="tanh")
The textbook 0.5 x (1 + tanh u) is not used: even in fp64, 1 + tanh u cancels to exactly 0 for dozens of negative bf16 inputs whose
true value is still a nonzero bf16 number (tests/test_epilogue_ref_cpu.py counts them)."""
import math

import torch

from vae_ref import BF16, F64, all_bf16, bf16_ulp, bits, rbf, steps  # noqa: F401  (re-exported for the tests)

FLUSH = 2.0 ** -126          # smallest normal fp32: v_exp_f32 / v_rcp_f32 flush results below it (csrc/common.h, umv_exp2)
ACT_MIN_EQUAL = 0.99         # the project's figure for kernels on v_exp_f32: share of bit-equal results outside the flush band


# ---- inputs: the 65 536 patterns and their permutations
def patterns(mult=1, offset=0):
    """all bf16 patterns, pattern (i * mult + offset) mod 65 536 at position i; an odd mult makes it a permutation"""
    assert mult % 2 == 1
    idx = (torch.arange(65536, dtype=torch.int64) * mult + offset) % 65536
    return all_bf16()[idx]


BIAS_MULT, BIAS_OFFSET = 257, 0        # bias = pattern 257 i: 256 exact ties, 254 exact cancellations, 1128 carries among (i, 257 i)
RES_MULT, RES_OFFSET = 129, 13849      # residual = pattern 129 i + 13849: 1010 ties, 636 sums in a lower binade (test_epilogue_ref_cpu.py counts them)


# ---- the steps
def accumulate(x_scale, w):
    """the fp32 accumulator of a one-hot row: 0 + x[m, 0] * W[n, 0] (+0 for a -0 weight: the accumulator starts at +0), as fp64"""
    return ((float(x_scale) * w.to(F64)) + 0.0).to(torch.float32).to(F64)


def add32(a64, b):
    """one fp32 addition, as fp64 (exact; overflow and inf - inf as in fp32)"""
    return (a64 + b.to(F64)).to(torch.float32).to(F64)


def silu_ideal(x):
    x = x.to(F64)
    return x / (1.0 + torch.exp(-x))


def gelu_ideal(x):
    x = x.to(F64)
    u = math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)
    return x / (1.0 + torch.exp(-2.0 * u))


IDEAL = {"silu": silu_ideal, "gelu_tanh": gelu_ideal}


def epilogue(acc64, bias=None, act=None, residual=None, out_f32=False):
    """the model of epi_store4 on an fp32 accumulator held as fp64.  Returns (out, pre): out is fp32 for out_f32 and bf16 otherwise
    (the IDEAL activation rounded once where act is set); pre is the bf16 pre-activation (None for out_f32)."""
    v = acc64 if bias is None else add32(acc64, bias)
    if out_f32:
        return v.to(torch.float32), None
    pre = rbf(v)
    v = pre
    if act is not None:
        v = rbf(IDEAL[act](pre))
    if residual is not None:
        v = rbf(v + residual.to(F64))
    return v.to(BF16), pre.to(BF16)


def swiglu(g64, u64):
    """(out, inner, gate): rbf(rbf(silu(rbf(g))) * rbf(u)) with the ideal SiLU, its inner value and the rounded gate, all bf16"""
    gate = rbf(g64)
    inner = rbf(silu_ideal(gate))
    return rbf(inner * rbf(u64)).to(BF16), inner.to(BF16), gate.to(BF16)


def product(inner_bf16, u64):
    """the outer step of SwiGLU on a given inner value: rbf(inner * rbf(u))"""
    return rbf(inner_bf16.to(F64) * rbf(u64)).to(BF16)


# ---- comparing
def value_class(t):
    """0 finite nonzero, 1 zero (either sign), 2 +inf, 3 -inf, 4 NaN"""
    f = t.to(F64)
    c = torch.zeros(f.shape, dtype=torch.int64, device=f.device)
    c = torch.where(f == 0, torch.ones_like(c), c)
    c = torch.where(torch.isposinf(f), torch.full_like(c, 2), c)
    c = torch.where(torch.isneginf(f), torch.full_like(c, 3), c)
    return torch.where(torch.isnan(f), torch.full_like(c, 4), c)


CLASS_NAMES = ("finite", "zero", "+inf", "-inf", "nan")


def canon_bits(t):
    """the bit patterns of a bf16 / fp32 tensor with every NaN mapped to one pattern (NaN <-> NaN: payload and sign are not compared)"""
    if t.dtype == BF16:
        b = bits(t).to(torch.int32) & 0xFFFF
        return torch.where(torch.isnan(t), torch.full_like(b, 0x7FC0), b)
    assert t.dtype == torch.float32
    b = t.contiguous().view(torch.int32)
    return torch.where(torch.isnan(t), torch.full_like(b, 0x7FC00000), b)


def count_diff(got, want):
    """number of elements whose bits differ (NaN <-> NaN equal, +0 and -0 different)"""
    assert got.shape == want.shape and got.dtype == want.dtype
    return int((canon_bits(got) != canon_bits(want)).sum())


def act_report(got, x, kind):
    """got = a kernel's bf16 activation of the bf16 inputs x (any shape): the figures check_act asserts on.
    finite: finite inputs; band: those in the flush band, |ideal| < 2^-126 * max(1, |x|), where the factor 1 / (1 + e) lies below the
    smallest normal fp32; differ: finite inputs outside the band whose result is not the rounded ideal; violations: finite inputs
    whose result is more than one bf16 value from the rounded ideal (outside the band) or not between zero and it (inside)."""
    got, x = got.reshape(-1).cpu(), x.reshape(-1).cpu()
    ideal = IDEAL[kind](x)
    want = rbf(ideal).to(BF16)
    fin = torch.isfinite(x.to(F64))
    band = fin & (ideal.abs() < FLUSH * x.to(F64).abs().clamp_min(1.0))
    st = steps(got, want)
    g64, w64 = got.to(F64), want.to(F64)
    in_band_ok = (g64 == 0) | ((torch.sign(g64) == torch.sign(w64)) & (g64.abs() <= w64.abs()))
    out = fin & ~band
    viol = (out & ~(torch.isfinite(g64) & (st <= 1))) | (band & ~in_band_ok)
    differ = out & (st != 0)
    n_out = int(out.sum())
    return {"finite": int(fin.sum()), "band": int(band.sum()), "differ": int(differ.sum()), "violations": int(viol.sum()),
            "equal_share": 1.0 if n_out == 0 else 1.0 - int(differ.sum()) / n_out,
            "worst": [float(v) for v in x.to(F64)[viol][:4]]}


def check_act(got, x, kind, what=""):
    """The acceptance rule for an activation on finite bf16 inputs: at most one bf16 value from the rounded ideal; in the flush band
    anything between zero and it inclusive (zeros of either sign equal); at least 99 % bit-equal outside the band."""
    r = act_report(got, x, kind)
    assert r["violations"] == 0, f"{what} {kind}: {r['violations']} inputs break the rule, e.g. x = {r['worst']}"
    assert r["equal_share"] >= ACT_MIN_EQUAL, f"{what} {kind}: only {r['equal_share']:.5f} bit-equal outside the flush band"
    return r


# ---- fp32 models of the device formula x * rcp(1 + exp2(t)), with exact exp2 and rcp and the hardware's flush to zero
def _formula(x, t64, clamp):
    x = x.to(F64)
    t = t64.to(torch.float32).to(F64)
    if clamp:
        t = t.clamp_max(126.0)                      # (fminf(NaN, 126) = 126 as well; NaN inputs are not compared)
    e = torch.exp2(t).to(torch.float32).to(F64)     # overflows to inf beyond 2^128
    e = torch.where(e < FLUSH, torch.zeros_like(e), e)
    r = (1.0 / (1.0 + e).to(torch.float32).to(F64)).to(torch.float32).to(F64)
    r = torch.where(r < FLUSH, torch.zeros_like(r), r)
    return rbf(x * r).to(BF16)


def silu_formula(x, clamp):
    """silu_f of gemm_epilogue.h; clamp=True: the form before the tail fix, exp2(min(t, 126))"""
    l2e = float(torch.tensor(1.4426950408889634, dtype=torch.float32))
    return _formula(x, -x.to(F64) * l2e, clamp)


def gelu_formula(x, clamp):
    """gelu_tanh_f of gemm_epilogue.h, fp32 step by step"""
    f32 = lambda v: v.to(torch.float32).to(F64)
    c0 = float(torch.tensor(-2.0 * 1.4426950408889634 * 0.7978845608028654, dtype=torch.float32))
    c1 = float(torch.tensor(c0, dtype=torch.float32) * torch.tensor(0.044715, dtype=torch.float32))
    x64 = x.to(F64)
    p = f32(c1 * f32(x64 * x64) + c0)               # fma: one rounding
    return _formula(x, x64 * p, clamp)
