"""Explicit reference models of the kernels in csrc/vae.hip and of the convolutions in csrc/vae_conv.hip (conv2d), on CPU tensors.

Every operation is computed in fp64 on bf16-rounded operands and rounded to bf16 exactly where the kernel's comment says a rounding
happens.  The rounding goes fp64 -> fp32 -> bf16, which is what the kernels do (one fp32 operation, then f2bf): the exact result of a
single + - * / on two fp32 values rounds to the same fp32 from fp64 as from the reals (53 >= 2 * 24 + 2), so each step equals the
kernel's fp32 step bit for bit, with no "fp32 emulation" in between.  Only exp is not exact on the device (about 1 fp32 ulp):
exp_near_tie() marks the inputs where that can move the bf16 result.

The VAE's constants (scale_factor, shift_factor) are fp32 values, float(np.float32(c)), as the kernels take them and as torch passes
a Python scalar to a device kernel.  torch on the CPU rounds the scalar of `bf16_tensor +- scalar` to bf16 first (and keeps fp32 for
* and /): tests/test_vae_ref_cpu.py pins that difference."""
import numpy as np
import torch

BF16 = torch.bfloat16
F64 = torch.float64


def c32(c):
    """a constant as the fp32 value a kernel argument carries"""
    return float(np.float32(c))


def rbf(x64):
    """fp64 -> fp32 -> bf16 -> fp64: the kernels' rbf() of an fp32 result"""
    return x64.to(torch.float32).to(BF16).to(F64)


def all_bf16():
    """all 65 536 bf16 patterns in pattern order"""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF16)


def bits(x):
    return x.contiguous().view(torch.int16)


def steps(a, b):
    """how many bf16 values lie between two bf16 tensors (0 = equal, 1 = neighbours; +0 and -0 count as one value)"""
    def order(x):
        i = bits(x).to(torch.int32) & 0xFFFF
        return torch.where(i >= 0x8000, -(i & 0x7FFF), i)
    return (order(a) - order(b)).abs()


def bf16_ulp(x):
    """the spacing of bf16 at |x| (fp64 tensor), 2^-133 for zero and subnormals"""
    a = x.to(F64).abs()
    e = torch.frexp(a)[1] - 1                                  # floor(log2 |x|); frexp(0) has exponent 0
    e = torch.where(a == 0, torch.full_like(e, -126), e)
    return torch.ldexp(torch.ones_like(a), e.clamp_min(-126) - 7)


# ---- the single steps: one fp64 operation on bf16 / fp32 operands, one rounding
def div_c(v, c):
    return rbf(v.to(F64) / c32(c))


def mul_c(v, c):
    return rbf(c32(c) * v.to(F64))


def add_c(v, c):
    return rbf(v.to(F64) + c32(c))


def sub_c(v, c):
    return rbf(v.to(F64) - c32(c))


# ---- one model per kernel
def nchw_to_nhwc(x, Cp):
    """[B,C,H,W] fp32 -> [B,H,W,Cp] bf16, pad channels +0"""
    B, C, H, W = x.shape
    out = torch.zeros((B, H, W, Cp), dtype=BF16)
    out[..., :C] = x.permute(0, 2, 3, 1).to(BF16)
    return out


def unpatchify_latent(tok_f32, h, w, p, c, scale, shift):
    """tokens [h*w, p*p*c] fp32 -> [h*p, w*p, c] bf16: bf16(bf16(bf16(tok) / scale) + shift), hwpqc -> (h p)(w q) c"""
    v = tok_f32.to(torch.float32).to(BF16)
    v = add_c(div_c(v, scale), shift).to(BF16)
    return v.view(h, w, p, p, c).permute(0, 2, 1, 3, 4).reshape(h * p, w * p, c).contiguous()


def pixels_u8(x_bf16):
    """trunc(bf16(clamp(bf16(bf16(x * 0.5) + 0.5), 0, 1) * 255)); NaN inputs are undefined"""
    v = rbf(rbf(x_bf16.to(F64) * 0.5) + 0.5).clamp(0.0, 1.0)
    return rbf(v * 255.0).trunc().nan_to_num(0.0).to(torch.uint8)


def latent_sample_patchify(mom, noise, b, h, w, p, scale, shift):
    """moments [B,Hm,Wm,2z] bf16 NHWC, noise [B,z,Hm,Wm] bf16 NCHW -> tokens [h*w, p*p*z] bf16 of sample b's top-left h*p x w*p window:
    bf16(scale * bf16(bf16(mean + bf16(bf16(exp(bf16(0.5 * logvar))) * noise)) - shift)), token order h w p q c; exp in fp64"""
    z = mom.shape[-1] // 2
    m = mom[b, :h * p, :w * p].to(F64)
    mean, logvar = m[..., :z], m[..., z:]
    nz = noise[b, :, :h * p, :w * p].permute(1, 2, 0).to(F64)
    std = rbf(torch.exp(rbf(0.5 * logvar)))
    zz = rbf(mean + rbf(std * nz))
    out = mul_c(sub_c(zz, shift), scale).to(BF16)
    return out.view(h, p, w, p, z).permute(0, 2, 1, 3, 4).reshape(h * w, p * p * z).contiguous()


def swish_chain(y_bf16):
    """bf16(y * bf16(sigmoid(y))) on a bf16 tensor.  sigmoid = 1 / (1 + exp(-y)) in fp64 with exp(-y) brought to fp32's range, as
    torch.sigmoid has it on a bf16 tensor: for y <= -89 the exponential is inf in fp32 and the sigmoid 0 (the product -0), where the
    real sigmoid is still a bf16 subnormal.  The kernel follows the reference there (gn_apply_kernel's comment)."""
    y = y_bf16.to(F64)
    e = torch.exp(-y).to(torch.float32).to(F64)
    return rbf(y * rbf(1.0 / (1.0 + e))).to(BF16)


def groupnorm_stats(x, eps):
    """fp64 (mean, rstd) per (sample, group) of x [B,HW,C], each broadcast to [B,HW,C]"""
    B, HW, C = x.shape
    xg = x.to(F64).view(B, HW, 32, C // 32)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True) + eps)
    return mean.expand_as(xg).reshape(B, HW, C), rstd.expand_as(xg).reshape(B, HW, C)


def groupnorm(x, gamma, beta, eps, swish):
    """x [B,HW,C] bf16 NHWC, 32 groups: fp64 mean and biased variance per (sample, group), y = bf16((x - mean) * rstd * gamma + beta)"""
    mean, rstd = groupnorm_stats(x, eps)
    y = rbf((x.to(F64) - mean) * rstd * gamma.to(F64) + beta.to(F64)).to(BF16)
    return swish_chain(y) if swish else y


def groupnorm_fp32_allowance(x, gamma, beta, eps):
    """how far an fp32 evaluation of (x - mean) * rstd * gamma + beta may lie from the exact value, per element, before its rounding
    to bf16.  fp32 statistics carry a relative error of about 2^-20 (1e-6): on the mean that moves the value by 2^-20 |mean| rstd |gamma|,
    and twice that on rstd (the variance is E[x^2] - mean^2, whose cancellation doubles the error for a sample whose mean exceeds its
    deviation), i.e. 2 * 2^-20 |x - mean| rstd |gamma|; the four fp32 operations add 4 * 2^-24 of the larger of the two terms.  With
    t = (|x| + |mean|) rstd |gamma| >= both |mean| rstd |gamma| and |x - mean| rstd |gamma|:  <= (1 + 2 + 1/4) 2^-20 max(t, |beta|)."""
    mean, rstd = groupnorm_stats(x, eps)
    t = (x.to(F64).abs() + mean.abs()) * rstd * gamma.to(F64).abs()
    return 3.25 * 2.0 ** -20 * torch.maximum(t, beta.to(F64).abs().expand_as(t))


def conv2d_out_hw(Hin, Win, ks, mode):
    """mode 0: the input's size; mode 1: twice it; mode 2: floor((n + 1 - 3) / 2) + 1 per axis, none for a single row or column"""
    if mode == 0:
        return Hin, Win
    if mode == 1:
        return 2 * Hin, 2 * Win
    return max((Hin + 1 - 3) // 2 + 1, 0), max((Win + 1 - 3) // 2 + 1, 0)


def conv2d_parts(x, w, bias=None, residual=None, mode=0):
    """umv_conv2d_nhwc_bf16 with the value before each rounding: (out bf16 [B,Hout,Wout,Cout], acc + bias fp64, . + residual fp64 or None).
    x [B,Hin,Win,Cin] bf16 NHWC, w [Cout,Cin,k,k] bf16 (as vae._Conv takes it), bias [Cout] bf16 or None, residual as the output or None.
    mode 0: stride 1, pad (k - 1) / 2.  mode 1: nearest 2x upsample, then pad 1.  mode 2: F.pad(0, 1, 0, 1), then stride 2 without padding.
    The sum runs in fp64 on the bf16 operands; the roundings are the kernels' (conv_epilogue4 and conv3x3_patch_kernel's copy of it):
    rbf(acc + bias), then rbf(. + residual) if there is a residual.  The sum itself is NOT rounded to fp32 here: the model is the kernels'
    bit for bit where the fp32 sum is exact in every order (tests/conv_cases.py builds such inputs), the exact convolution otherwise."""
    Cout, Cin, ks, _ = w.shape
    B, Hin, Win, _ = x.shape
    assert x.shape[3] == Cin and w.shape[2] == w.shape[3] and mode in (0, 1, 2)
    Hout, Wout = conv2d_out_hw(Hin, Win, ks, mode)
    if B * Hout * Wout == 0:
        return torch.zeros((B, Hout, Wout, Cout), dtype=BF16), torch.zeros((B, Hout, Wout, Cout), dtype=F64), None
    xc, w64 = x.to(F64).permute(0, 3, 1, 2), w.to(F64)
    if mode == 0:
        acc = torch.nn.functional.conv2d(xc, w64, padding=(ks - 1) // 2)
    elif mode == 1:
        acc = torch.nn.functional.conv2d(xc.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3), w64, padding=1)
    else:
        acc = torch.nn.functional.conv2d(torch.nn.functional.pad(xc, (0, 1, 0, 1)), w64, stride=2)
    acc = acc.permute(0, 2, 3, 1)
    assert tuple(acc.shape) == (B, Hout, Wout, Cout)
    pre1 = acc + (bias.to(F64) if bias is not None else 0.0)
    v = rbf(pre1)
    pre2 = None
    if residual is not None:
        pre2 = v + residual.to(F64)
        v = rbf(pre2)
    return v.to(BF16).contiguous(), pre1, pre2


def conv2d(x, w, bias=None, residual=None, mode=0):
    """the model of umv_conv2d_nhwc_bf16: conv2d_parts' first result"""
    return conv2d_parts(x, w, bias, residual, mode)[0]


def bf16_inexact(v64):
    """mask of the fp64 values that are no bf16 value: rounding them changes them"""
    return rbf(v64) != v64


def bf16_tie(v64):
    """mask of the fp64 values exactly half way between two neighbouring bf16 values, where round-to-nearest-even decides"""
    return (rbf(v64) - v64).abs() * 2 == bf16_ulp(v64)


def softmax_rows(S, scale):
    """(P_exact fp64, l fp64): exp((S - rowmax) * scale); an all -inf row gives zeros and l = 0"""
    s = S.to(F64)
    mx = s.max(-1, keepdim=True).values
    mx = torch.where(torch.isinf(mx) & (mx < 0), torch.zeros_like(mx), mx)
    P = torch.exp((s - mx) * float(scale))
    return P, P.sum(-1)


def rowscale(O, l):
    """O / l in fp64, zeros where l <= 0"""
    l64 = l.to(F64)[:, None]
    return torch.where(l64 > 0, O.to(F64) / l64, torch.zeros((), dtype=F64))


def exp_near_tie(x_bf16, ulps_f32=2):
    """mask of the inputs whose exact exp(x) lies within ulps_f32 fp32 ulps of the midpoint between two neighbouring bf16 values: an
    exponential that is correct to 1 fp32 ulp may land on either neighbour there.  (Results of 0 and inf are never ties.)"""
    e = torch.exp(x_bf16.to(F64))
    ok = torch.isfinite(e) & (e > 0)
    e = torch.where(ok, e, torch.ones_like(e))
    ex = (torch.frexp(e)[1] - 1).clamp_min(-126)               # the fp32 exponent of e; subnormals share 2^-126's spacing
    frac = torch.ldexp(e, 23 - ex)                             # e in fp32 ulps, exact
    r = frac - torch.floor(frac / 65536.0) * 65536.0           # position inside one bf16 step (65 536 fp32 ulps)
    return ok & ((r - 32768.0).abs() <= ulps_f32)
