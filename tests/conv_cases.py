"""The shapes and the data of the convolution tests, shared by tests/test_vae_ref_cpu.py (which checks the conditions the data must meet)
and tests/test_vae_conv_gpu.py (which holds conv_tiled_kernel and conv3x3_patch_kernel of csrc/vae_conv.hip to vae_ref.conv2d bit for bit).

Exact-grid inputs.  x is an integer in [-8, 8], weights and bias are k / 8 with |k| <= 16, the residual is k / 8 with |k| <= 64; x is then
multiplied by 2^ex, the weight by 2^ew, bias and residual by 2^(ex + ew), which keeps every tensor on one common grid and gives the
magnitudes the model has (exactness does not depend on the scale: a power of two moves no mantissa).  Every product is a multiple of
unit = 2^(ex + ew) / 64 and every partial sum of any subset of them an integer count of that unit; test_vae_ref_cpu.py checks that the
largest count any order can reach, sum |x||w| + |bias| + |residual|, stays below 2^22 for every case.  So every fp32 summation order - and
an MFMA accumulator that truncates instead of rounding - gives the exact sum, acc + bias and . + residual are exact in fp32, and the
only roundings are the two to bf16 that the model reproduces."""
from collections import namedtuple

import torch

import vae_ref as R

BF16 = torch.bfloat16

Case = namedtuple("Case", "ks mode Cin Cout B Hin Win bias res seed ex ew")

# (ex, ew) by case index: unit scale, the model's magnitudes (activations of a few units, weights of a few hundredths), and both ends of the
# range 2^-12 .. 2^12
_SCALES = [(0, 0), (-2, -5), (-12, 12), (12, -12), (-1, -7), (12, 12), (-12, -12), (-3, -4)]


def _table(rows, seed0):
    out = []
    for i, (shape, flags, *seed) in enumerate(rows):
        ex, ew = _SCALES[(seed0 + i) % len(_SCALES)]
        out.append(Case(*shape, "b" in flags, "r" in flags, seed[0] if seed else seed0 + i, ex, ew))
    return out


# (ks, mode, Cin, Cout, B, Hin, Win), "b" = with a bias, "r" = with a residual[, a seed of its own: the few outputs of a one-pixel image hold
# a tie and enough inexact sums only for some draws]
# ---- conv_tiled_kernel, 16 (n) x 256 (m) tile: Cout <= 16, k-step 128, 2 buffers
GATHER_16x256 = _table([
    ((3, 0, 8, 16, 1, 3, 5), "br"),         # M = 15 < 16; one k-step; a k-tile spanning four taps
    ((3, 0, 128, 3, 2, 20, 20), "br"),      # ragged last 256-row block; scalar epilogue with 3 valid channels
    ((3, 0, 64, 6, 1, 9, 9), "r"),          # KT = 18: the last step half past KT
    ((1, 0, 32, 13, 1, 16, 17), "b"),       # 1 x 1, KT = 1, odd Cout
    ((3, 2, 16, 8, 2, 7, 6), ""),           # downsample into a small Cout
    ((3, 1, 96, 16, 2, 9, 13), ""),         # upsample into Cout = 16
], 100)
# ---- conv_tiled_kernel, 128 (n) x 64 (m) tile: the default, k-step 64, 3 buffers; 1, 2, 3, 4 and more steps reach each arm of the `ahead` wait
GATHER_128x64 = _table([
    ((1, 0, 8, 20, 1, 5, 5), "b"),          # KT = 1
    ((1, 0, 64, 128, 1, 8, 8), "br"),       # one step
    ((3, 0, 8, 32, 2, 9, 9), ""),           # two steps
    ((1, 0, 160, 36, 1, 8, 9), "r"),        # three steps, wave-uniform tap path
    ((3, 0, 24, 17, 2, 6, 7), "br"),        # four steps, per-lane tap path, Cout % 4 != 0
    ((3, 0, 48, 130, 1, 8, 8), "br"),       # per-lane tap path; scalar epilogue with 2 valid channels in the last group
    ((3, 0, 256, 132, 1, 17, 15), "b"),     # M = 255; a second n-block of 4 channels with 7 invalid weight tiles
    ((3, 1, 32, 36, 2, 1, 1), "b"),
    ((3, 1, 16, 64, 1, 6, 10), "br"),
    ((3, 2, 32, 32, 2, 2, 2), "b"),
    ((3, 2, 32, 32, 1, 3, 3), ""),
    ((3, 2, 8, 40, 2, 15, 11), "br"),
    ((3, 2, 64, 64, 1, 16, 12), "r"),
], 200)
# ---- conv_tiled_kernel, 128 x 128 tile: 130 x 3 >= 384 workgroups; KT = 9 (odd), ragged last row block.  With B = 1 the same shape has 195
#      workgroups and takes the 128 x 64 tile
GATHER_128x128 = _table([((3, 0, 32, 384, 2, 91, 91), "br")], 300)
# ---- conv3x3_patch_kernel (| 16), mode 0: one to four 64-channel slices; tiles of 1, 15, 16, 17 and 33 pixels; Cout below, at, just above 128
PATCH_0 = _table([
    ((3, 0, 64, 4, 1, 1, 1), "b", 8),       # four outputs: 39.125 (a tie), 11.375, -34.625 (a tie), 9.75
    ((3, 0, 64, 128, 2, 16, 16), "br"),
    ((3, 0, 128, 36, 3, 17, 15), "r"),
    ((3, 0, 192, 132, 1, 15, 33), "b"),
    ((3, 0, 256, 128, 2, 3, 40), "br"),
    ((3, 0, 64, 260, 1, 33, 17), ""),
], 400)
# ---- conv3x3_patch_kernel (| 16), mode 1
PATCH_1 = _table([
    ((3, 1, 64, 64, 1, 1, 1), "b"),
    ((3, 1, 64, 128, 2, 8, 8), "br"),
    ((3, 1, 128, 36, 3, 9, 5), ""),
    ((3, 1, 192, 132, 1, 5, 20), "r"),
    ((3, 1, 256, 4, 2, 12, 9), "b"),
], 500)

CASES = GATHER_16x256 + GATHER_128x64 + GATHER_128x128 + PATCH_0 + PATCH_1


def case_id(c):
    return f"k{c.ks}m{c.mode}-{c.Cin}to{c.Cout}-{c.B}x{c.Hin}x{c.Win}" + ("-b" if c.bias else "") + ("-r" if c.res else "")


def patch_ok(ks, mode, Cin, Cout):
    """where the entry point lets conv3x3_patch_kernel run (| 16 is UMV_ERR_UNSUPPORTED elsewhere); pointers are 8-byte aligned in the tests"""
    return ks == 3 and mode in (0, 1) and Cin % 64 == 0 and Cout % 4 == 0


def variants(c):
    """the mode arguments a case runs with: the policy, | 32 = the gather kernel, | 16 = the input-stationary kernel where it can run"""
    return [c.mode, c.mode | 32] + ([c.mode | 16] if patch_ok(c.ks, c.mode, c.Cin, c.Cout) else [])


def _grid(shape, lim, scale, g):
    v = torch.randint(-lim, lim + 1, shape, generator=g).to(torch.float64) * scale
    assert bool((v.to(BF16).to(torch.float64) == v).all())
    return v.to(BF16)


def make_inputs(c):
    """(x [B,Hin,Win,Cin], w [Cout,Cin,ks,ks], bias [Cout] or None, residual [B,Hout,Wout,Cout] or None) bf16, and the grid's unit"""
    g = torch.Generator().manual_seed(c.seed)
    sx, sw = 2.0 ** c.ex, 2.0 ** c.ew
    Hout, Wout = R.conv2d_out_hw(c.Hin, c.Win, c.ks, c.mode)
    x = _grid((c.B, c.Hin, c.Win, c.Cin), 8, sx, g)
    w = _grid((c.Cout, c.Cin, c.ks, c.ks), 16, sw / 8, g)
    bias = _grid((c.Cout,), 16, sx * sw / 8, g) if c.bias else None
    res = _grid((c.B, Hout, Wout, c.Cout), 64, sx * sw / 8, g) if c.res else None
    return x, w, bias, res, sx * sw / 64


def normal_bf16_draw(n, seed):
    """n values drawn without repetition, in shuffled order, from all normal finite bf16 values and the two zeros (no subnormals, no inf, no NaN)"""
    v = R.all_bf16()
    e = (R.bits(v).to(torch.int32) >> 7) & 0xFF
    pool = v[((e >= 1) & (e <= 254)) | ((R.bits(v).to(torch.int32) & 0x7FFF) == 0)]
    assert pool.numel() == 2 * 254 * 128 + 2 and n <= pool.numel()
    return pool[torch.randperm(pool.numel(), generator=torch.Generator().manual_seed(seed))[:n]].clone()


def one_hot_weight(C, tap):
    """[C, C, 3, 3]: 1 where ci == co at filter tap `tap` = ky * 3 + kx, 0 elsewhere - the convolution moves the image by the tap"""
    w = torch.zeros((C, C, 3, 3), dtype=BF16)
    w[torch.arange(C), torch.arange(C), tap // 3, tap % 3] = 1.0
    return w
