"""The two implicit-GEMM convolutions of csrc/vae_conv.hip - conv_tiled_kernel (the gather kernel, three tile shapes) and
conv3x3_patch_kernel (input-stationary, modes 0 and 1) - against vae_ref.conv2d, BIT FOR BIT, at the smallest shapes that reach each
branch: tests/conv_cases.py holds the shapes and the exact-grid data and says why every fp32 summation order gives the exact sum on
them (tests/test_vae_ref_cpu.py checks those conditions and the model itself).  The only roundings are the epilogue's two to bf16, which
the model reproduces, so there is no tolerance: gather kernel, patch kernel and model agree in every bit (+0 and -0 count as one value).

Every call goes straight to umv_conv2d_nhwc_bf16 with weights packed by vae._Conv, in up to three variants: the dispatch policy (mode),
mode | 32 (the gather kernel) and, where the entry allows it, mode | 16 (the input-stationary kernel).  The output is a Guarded buffer:
every element must be written and both guards stay intact.  The input lies inside a larger allocation whose frame of bf16 NaN is at
least (Win + 2) * Cin elements on either side, so a tap taken from outside the image - the row above, the neighbouring image of the
batch - turns a sum into NaN instead of a plausible number, and stays inside allocated memory."""
import functools

import pytest
import torch

import conv_cases as CC
import vae_ref as R
from guarded import Guarded

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
ERR_ARG, ERR_UNSUPPORTED = -1, -3


def _lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd import _lib, ops
    return _lib.load(), ops._stream


def _framed(x):
    """x [B,H,W,C] on the device inside a frame of NaN: (the allocation, the address of x in it)"""
    B, H, W, C = x.shape
    pad = max((W + 2) * C, 64)                                 # a multiple of 8 elements: x stays 16-byte aligned
    raw = torch.full((x.numel() + 2 * pad,), float("nan"), dtype=BF16, device="cuda")
    raw[pad:pad + x.numel()] = x.reshape(-1).cuda()
    return raw, raw[pad:].data_ptr()


class _Call:
    """one convolution's operands on the device; run(mode argument) -> (return code, Guarded output)"""

    def __init__(self, x, w, bias, res, mode):
        from unimedvl_amd.vae import _Conv
        self.lib, self.stream = _lib()
        self.conv = _Conv(w, bias, "cuda")
        self.B, self.Hin, self.Win, self.Cin = x.shape
        self.Cout, self.ks, self.mode = w.shape[0], w.shape[2], mode
        self.xraw, self.xptr = _framed(x)
        self.res = None if res is None else res.contiguous().cuda()
        self.oshape = (self.B, *R.conv2d_out_hw(self.Hin, self.Win, self.ks, mode), self.Cout)

    def run(self, mv):
        out = Guarded(self.oshape[0] * self.oshape[1] * self.oshape[2] * self.oshape[3], BF16)
        rc = self.lib.umv_conv2d_nhwc_bf16(self.xptr, self.conv.lin.wp.data_ptr(), None if self.conv.bias is None else self.conv.bias.data_ptr(),
                                           None if self.res is None else self.res.data_ptr(), out.ptr(), self.B, self.Cin, self.Hin, self.Win,
                                           self.Cout, self.ks, mv, self.stream())
        return rc, out

    def result(self, mv):
        rc, out = self.run(mv)
        assert rc == 0, f"mode {mv}: rc {rc}: {self.lib.umv_last_error().decode()}"
        got, raw = out.fetch()
        left = int((raw == out.pat).sum())
        assert left == 0, f"mode {mv}: {left} of {raw.numel()} output elements were not written"
        return got.view(self.oshape)


def _hold(got, ref, what):
    """got == ref bit for bit (+-0 one value), or fail with where the difference lies"""
    ne = R.steps(got, ref) != 0
    if not bool(ne.any()):
        return
    B, H, W, C = ref.shape
    idx = ne.nonzero()
    b, y, x, ch = idx[0].tolist()
    ib, ys, xs, cs = idx.unbind(1)
    m = (ib * H + ys) * W + xs
    border = (ys == 0) | (ys == H - 1) | (xs == 0) | (xs == W - 1)
    tile = (m % 16 == 0) | (m % 16 == 15) | (ys % 16 == 0) | (ys % 16 == 15) | (xs % 16 == 0) | (xs % 16 == 15)
    tail = (cs >= C // 16 * 16) | (cs >= C // 4 * 4)
    pytest.fail(f"{what}: {idx.shape[0]} of {ne.numel()} elements differ, first at (b, y, x, channel) = ({b}, {y}, {x}, {ch}): "
                f"{float(got[b, y, x, ch])} != {float(ref[b, y, x, ch])}; {int(torch.isnan(got.float()).sum())} are NaN; of the differing "
                f"{int(border.sum())} on an image border, {int(tile.sum())} on a 16-pixel tile border (flat or 2-D), "
                f"{int(tail.sum())} in a channel-group tail (the last partial 16 or 4 of {C})")


@functools.lru_cache(maxsize=None)
def _case(c):
    x, w, bias, res, _ = CC.make_inputs(c)
    return x, w, bias, res, R.conv2d(x, w, bias, res, c.mode)


# ----------------------------------------------------------------------------- the case table
@pytest.mark.parametrize("c", CC.CASES, ids=CC.case_id)
def test_conv_equals_the_model(c):
    x, w, bias, res, ref = _case(c)
    call = _Call(x, w, bias, res, c.mode)
    assert call.oshape == tuple(ref.shape)
    for mv in CC.variants(c):
        _hold(call.result(mv), ref, f"{CC.case_id(c)} mode {mv}")


def _batch_and_its_images(x, w, bias, res, what):
    both = _Call(x, w, bias, res, 0).result(0)
    for b in range(x.shape[0]):
        one = _Call(x[b:b + 1], w, bias, None if res is None else res[b:b + 1], 0).result(0)
        _hold(one, both[b:b + 1], f"{what}: image {b} alone against the batch")
    return both


def test_a_batch_equals_its_images_where_the_tile_depends_on_the_batch():
    """(3,0,32,384,2,91,91) runs 390 workgroups of the 128 x 128 tile, each of its images alone 195 of the 128 x 64 tile: the one place
    where the choice of kernel depends on the batch.  Both tiles take k in steps of 64 in the same order, so "a batch equals its images
    one by one" holds bit for bit, on grid inputs (and equals the model) and on randn inputs"""
    (c,) = CC.GATHER_128x128
    x, w, bias, res, ref = _case(c)
    _hold(_batch_and_its_images(x, w, bias, res, "grid inputs"), ref, "grid inputs: the batch against the model")
    g = torch.Generator().manual_seed(310)
    rn = lambda shape, s: (torch.randn(shape, generator=g) * s).to(BF16)
    x, w = rn(x.shape, 1.0), rn(w.shape, 1 / (3 * c.Cin ** 0.5))
    bias, res = rn(bias.shape, 0.1), rn(res.shape, 1.0)
    both = _batch_and_its_images(x, w, bias, res, "randn inputs")
    assert bool(torch.isfinite(both.float()).all())
    exact = R.conv2d(x, w, bias, res, 0)
    assert float((both.double() - exact.double()).abs().max()) <= 2.0 ** -6 * float(exact.double().abs().max())   # the same data, not garbage


# ----------------------------------------------------------------------------- one-hot weights, real data
SHIFT_B, SHIFT_H, SHIFT_W = 2, 17, 15


@functools.lru_cache(maxsize=None)
def _shift_x(C):
    return CC.normal_bf16_draw(SHIFT_B * SHIFT_H * SHIFT_W * C, 70 + C).view(SHIFT_B, SHIFT_H, SHIFT_W, C)


def _shift_variants(C, mode):
    return [mode, mode | 32] + ([mode | 16] if CC.patch_ok(3, mode, C, C) else [])


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("C", [64, 8])
def test_one_hot_weights_move_the_image_by_the_tap(C, mode):
    """W[co][tap][ci] = 1 iff ci == co, for each of the nine taps: the output is the input moved by the tap, zeros where the tap falls
    outside, nothing from the other image of the batch.  x is a shuffled draw from all normal finite bf16 values and zeros (subnormals are
    not this test's subject), so every bf16 exponent goes through the data path unchanged and a wrong address shows at once"""
    x = _shift_x(C)
    for tap in range(9):
        w = CC.one_hot_weight(C, tap)
        ref = R.conv2d(x, w, None, None, mode)
        if mode == 0:                                         # the model's statement, spelled out once more where it is simplest
            ky, kx = tap // 3, tap % 3
            moved = torch.zeros_like(x)
            ys = [y for y in range(SHIFT_H) if 0 <= y + ky - 1 < SHIFT_H]
            xs = [v for v in range(SHIFT_W) if 0 <= v + kx - 1 < SHIFT_W]
            moved[:, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = x[:, ys[0] + ky - 1:ys[-1] + ky, xs[0] + kx - 1:xs[-1] + kx]
            assert bool((R.steps(ref, moved) == 0).all())
        call = _Call(x, w, None, None, mode)
        for mv in _shift_variants(C, mode):
            _hold(call.result(mv), ref, f"one-hot tap {tap}, C = {C}, mode {mv}")


def test_one_hot_weights_with_bias_and_residual():
    """mode 0 once more with a bias and a residual drawn from the same set: rbf(x moved + bias), then rbf(. + residual), over all exponents"""
    C = 64
    x = _shift_x(C)
    bias = CC.normal_bf16_draw(C, 81)
    res = CC.normal_bf16_draw(x.numel(), 82).view(x.shape)
    for tap in range(9):
        w = CC.one_hot_weight(C, tap)
        ref = R.conv2d(x, w, bias, res, 0)
        assert not bool(torch.isnan(ref.float()).any())
        call = _Call(x, w, bias, res, 0)
        for mv in _shift_variants(C, 0):
            _hold(call.result(mv), ref, f"one-hot tap {tap} with bias and residual, mode {mv}")


# ----------------------------------------------------------------------------- arguments: none of these launches a kernel
def _arg_call(B, Cin, Hin, Win, Cout, ks, mv, n_out=0):
    lib, stream = _lib()
    x = torch.zeros((max(B, 1) * max(Hin, 1) * max(Win, 1) * max(Cin, 8) + 4096,), dtype=BF16, device="cuda")
    wp = torch.zeros((1 << 16,), dtype=BF16, device="cuda")       # more than any packed image of these shapes
    out = Guarded(n_out, BF16)
    rc = lib.umv_conv2d_nhwc_bf16(x.data_ptr(), wp.data_ptr(), None, None, out.ptr(), B, Cin, Hin, Win, Cout, ks, mv, stream())
    return rc, out


@pytest.mark.parametrize("Hin,Win", [(1, 3), (3, 1), (1, 1)])
def test_downsample_of_one_row_or_column_is_empty(Hin, Win):
    """floor((n + 1 - 3) / 2) + 1 = 0 for n = 1, as vae.py sizes the output: UMV_OK and nothing written.  (Truncating division gave one row:
    8 elements for (1, 3), which fit inside the guard, so this test stays inside allocated memory on either side of the fix.)"""
    for mv in (2, 2 | 32):
        rc, out = _arg_call(1, 8, Hin, Win, 8, 3, mv)
        assert rc == 0
        assert out.untouched()


@pytest.mark.parametrize("mode", [1, 2, 1 | 32, 2 | 32, 1 | 16])
def test_a_1x1_convolution_is_stride_1_only(mode):
    rc, out = _arg_call(1, 64, 4, 4, 64, 1, mode, n_out=4 * 4 * 64)
    assert rc == ERR_UNSUPPORTED
    assert out.untouched()


@pytest.mark.parametrize("B,Hin,Win,Cout", [(-1, 4, 4, 8), (1, -4, 4, 8), (1, 4, -4, 8), (1, 4, 4, -8), (1, 4, 4, 0), (-1, -4, 4, 8)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_negative_sizes_are_rejected(B, Hin, Win, Cout, mode):
    rc, out = _arg_call(B, 8, Hin, Win, Cout, 3, mode, n_out=256)
    assert rc == ERR_ARG
    assert out.untouched()


@pytest.mark.parametrize("Cin,Cout,ks,mode", [(32, 64, 3, 0), (64, 6, 3, 0), (64, 64, 3, 2), (64, 64, 1, 0), (96, 64, 3, 1)])
def test_forcing_the_patch_kernel_where_it_cannot_run_is_an_error(Cin, Cout, ks, mode):
    rc, out = _arg_call(1, Cin, 4, 4, Cout, ks, mode | 16, n_out=8 * 8 * 64)
    assert rc == ERR_UNSUPPORTED
    assert out.untouched()
