"""Every kernel of csrc/vae.hip, one small launch per case, against the explicit models of tests/vae_ref.py (the convolutions of
csrc/vae_conv.hip are held to the same file's conv2d in tests/test_vae_conv_gpu.py).  The models: fp64 per operation, bf16 roundings
where the kernels' comments put them; tests/test_vae_ref_cpu.py checks the models themselves.  Scalar chains are walked over EVERY bf16 value; layouts at h != w, crops of the latent and b > 0.  Outputs are prefilled
with a NaN pattern and framed by guard elements: nothing outside the result may be written.

Where exact equality of bits is not the contract, the bound is derived, not measured:
  - expf on the device is correct to about 1 fp32 ulp: only inputs that vae_ref.exp_near_tie flags (exact exp within 2 fp32 ulps of a
    bf16 midpoint; at most two half-log-variances exist, test_vae_ref_cpu.py) may land on the neighbouring bf16 value, and a
    subnormal result may be off by one subnormal step;
  - GroupNorm's fp32 statistics, the softmax's v_exp_f32 and the row scale's fp32 reciprocal carry relative errors of 1e-6 ... 5e-6
    against a bf16 half-ulp of 2^-9: at most the neighbouring bf16 value, and 99 % (99.9 %) of all elements exactly the model's.
    A GroupNorm output that cancels far below its terms is held to the fp32 chain's derived error instead (test_groupnorm_against_fp64)."""
import pytest
import torch

import vae_ref as R
from guarded import Guarded

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SCALE, SHIFT = 0.3611, 0.1159


def _lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd import _lib, ops
    return _lib.load(), ops._stream


def _randn(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _same_bits(got, ref, what):
    ne = R.bits(got) != R.bits(ref)
    assert not bool(ne.any()), f"{what}: {int(ne.sum())} of {ne.numel()} differ, first at {ne.flatten().nonzero()[0].item()}"


# ----------------------------------------------------------------------------- umv_nchw_f32_to_nhwc_bf16
@pytest.mark.parametrize("B,C,H,W,Cp", [(2, 3, 5, 7, 8), (1, 3, 4, 4, 3), (2, 1, 1, 300, 8)])
def test_nchw_to_nhwc(B, C, H, W, Cp):
    lib, stream = _lib()
    x = _randn((B, C, H, W), 11) * 3                                       # 24-bit mantissas: every value needs rounding
    special = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), 1e-40, -3e-39, 1.00390625, 1.01171875, 3.4028234663852886e38])
    x.view(-1)[:special.numel()] = special                                  # +-0, +-inf, denormals, two ties, the round-up to inf
    x.view(-1)[-1] = -0.0
    out = Guarded(B * H * W * Cp, BF16)
    xd = x.cuda()
    assert lib.umv_nchw_f32_to_nhwc_bf16(xd.data_ptr(), out.ptr(), B, C, H, W, Cp, stream()) == 0
    got, _ = out.fetch()
    ref = R.nchw_to_nhwc(x, Cp)
    _same_bits(got.view(B, H, W, Cp), ref, "nchw -> nhwc")
    assert bool((R.bits(got.view(B, H, W, Cp)[..., C:]) == 0).all()), "pad channels must be +0"


def test_nchw_to_nhwc_rejects_fewer_channels_than_the_image():
    lib, stream = _lib()
    xd = torch.zeros((1, 3, 4, 4), device="cuda")
    out = Guarded(4 * 4 * 3, BF16)
    assert lib.umv_nchw_f32_to_nhwc_bf16(xd.data_ptr(), out.ptr(), 1, 3, 4, 4, 2, stream()) != 0
    assert out.untouched()


# ----------------------------------------------------------------------------- umv_unpatchify_latent
def _unpatchify(tok, h, w, p, c, scale, shift):
    lib, stream = _lib()
    out = Guarded(h * p * w * p * c, BF16)
    td = tok.cuda()
    assert lib.umv_unpatchify_latent(td.data_ptr(), out.ptr(), h, w, p, c, scale, shift, stream()) == 0
    return out.fetch()[0].view(h * p, w * p, c)


def test_unpatchify_every_bf16_value():
    """all 65 536 patterns as fp32 tokens in one call: the rounding chain with the fp32 shift, and the layout at p = 2"""
    h = w = 32
    tok = R.all_bf16().float().view(h * w, 2 * 2 * 16)
    got = _unpatchify(tok, h, w, 2, 16, SCALE, SHIFT)
    ref = R.unpatchify_latent(tok, h, w, 2, 16, SCALE, SHIFT)
    nan = torch.isnan(ref.float())
    assert int(nan.sum()) == 65536 - 65280 - 2                            # the NaN patterns; +-inf / scale + shift stays inf
    assert bool(torch.isnan(got.float())[nan].all()), "NaN must give NaN"
    _same_bits(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(ref), ref), "unpatchify, all bf16")


@pytest.mark.parametrize("h,w,p,c,scale,shift", [(3, 5, 2, 16, SCALE, SHIFT), (5, 3, 2, 4, SCALE, SHIFT), (7, 1, 1, 16, SCALE, SHIFT),
                                                  (1, 1, 2, 16, SCALE, SHIFT), (3, 5, 2, 16, 1.5305, 0.0609), (5, 3, 2, 4, 1.0, 0.0)])
def test_unpatchify_layout_and_constants(h, w, p, c, scale, shift):
    tok = _randn((h * w, p * p * c), 21) * 1.7                              # fp32 values that are not bf16: the first rounding counts
    assert bool((tok.to(BF16).float() != tok).any())
    got = _unpatchify(tok, h, w, p, c, scale, shift)
    _same_bits(got, R.unpatchify_latent(tok, h, w, p, c, scale, shift), f"unpatchify {(h, w, p, c, scale, shift)}")


# ----------------------------------------------------------------------------- umv_pixels_to_u8
def _pixels(x, npix, Cs):
    lib, stream = _lib()
    out = Guarded(npix * 3, torch.uint8)
    xd = x.cuda()
    assert lib.umv_pixels_to_u8(xd.data_ptr(), out.ptr(), npix, Cs, stream()) == 0
    return out.fetch()[0]


@pytest.mark.parametrize("Cs,fill", [(8, 300.0), (8, float("nan")), (3, None)])
def test_pixels_every_bf16_value(Cs, fill):
    """all 65 536 patterns in the first three channels of 21 846 pixels; the other channels hold a value that would show if read"""
    npix = 21846
    v = torch.zeros(npix * 3, dtype=BF16)
    v[:65536] = R.all_bf16()
    x = torch.full((npix, Cs), 0.0 if fill is None else fill, dtype=BF16)
    x[:, :3] = v.view(npix, 3)
    got = _pixels(x, npix, Cs)
    ref = R.pixels_u8(v)
    ok = ~torch.isnan(v.float())
    assert int(ok.sum()) == 65280 + 2 + 2
    ne = (got != ref) & ok
    assert not bool(ne.any()), f"{int(ne.sum())} values differ, e.g. {float(v[ne][0])}: {int(got[ne][0])} != {int(ref[ne][0])}"
    assert torch.unique(got[ok]).numel() == 256


@pytest.mark.parametrize("npix", [1, 85, 86])
def test_pixels_small_counts(npix):
    """255 and 258 output bytes: the last block's bound, with the guard bytes behind it"""
    x = (_randn((npix, 8), 31) * 0.8).to(BF16)
    x[:, 3:] = float("nan")
    got = _pixels(x, npix, 8)
    assert torch.equal(got, R.pixels_u8(x[:, :3].reshape(-1)))


def test_pixels_rejects_fewer_than_three_channels():
    lib, stream = _lib()
    xd = torch.zeros((4, 2), dtype=BF16, device="cuda")
    out = Guarded(12, torch.uint8)
    assert lib.umv_pixels_to_u8(xd.data_ptr(), out.ptr(), 4, 2, stream()) != 0
    assert out.untouched()


# ----------------------------------------------------------------------------- umv_latent_sample_patchify
def _sample(mom, noise, b, h, w, p, scale, shift):
    lib, stream = _lib()
    B, Hm, Wm, z2 = mom.shape
    out = Guarded(h * w * p * p * (z2 // 2), BF16)
    md, nd = mom.cuda(), noise.cuda()
    assert lib.umv_latent_sample_patchify(md.data_ptr(), nd.data_ptr(), out.ptr(), b, Hm, Wm, z2 // 2, h, w, p, scale, shift, stream()) == 0
    return out.fetch()[0].view(h * w, p * p * (z2 // 2))


def test_latent_sample_every_log_variance():
    """every finite bf16 log-variance through mean = 0, noise = 1, scale = 1, shift = 0: the result is bf16(exp(bf16(0.5 * logvar)))"""
    z, Hm = 16, 64
    lv = R.all_bf16()
    lv = torch.where(torch.isfinite(lv.float()), lv, torch.zeros_like(lv))
    mom = torch.zeros((1, Hm, Hm, 2 * z), dtype=BF16)
    mom[0, :, :, z:] = lv.view(Hm, Hm, z)
    noise = torch.ones((1, z, Hm, Hm), dtype=BF16)
    got = _sample(mom, noise, 0, Hm, Hm, 1, 1.0, 0.0).view(-1)
    ref = R.latent_sample_patchify(mom, noise, 0, Hm, Hm, 1, 1.0, 0.0).view(-1)
    half = (0.5 * lv.double()).to(BF16)
    tie = R.exp_near_tie(half)
    assert torch.unique(R.bits(half[tie])).numel() <= 2
    small = ref.double().abs() < 2.0 ** -126                               # subnormal results and the underflow to 0
    ne = R.bits(got) != R.bits(ref)
    strict = ~small & ~tie
    print(f"latent sample over {lv.numel()} log-variances: {int((ne & strict).sum())} of {int(strict.sum())} normal / inf results differ; "
          f"exemptions taken: {int((ne & tie).sum())} of {int(tie.sum())} exp ties, {int((ne & small & ~tie).sum())} of {int(small.sum())} "
          f"subnormal results one step off")
    assert not bool((ne & strict).any()), f"{int((ne & strict).sum())} normal results differ, first log-variance {float(lv[ne & strict][0])}"
    assert bool((R.steps(got, ref)[tie] <= 1).all())
    assert bool(((got.double() - ref.double()).abs()[small] <= 2.0 ** -133).all()), "a subnormal result is more than one step off"


@pytest.mark.parametrize("b", [0, 1])
@pytest.mark.parametrize("Hm,Wm,z,h,w,p", [(12, 20, 16, 5, 9, 2), (12, 20, 16, 6, 10, 2), (9, 7, 4, 9, 7, 1), (6, 6, 16, 1, 1, 2)])
def test_latent_sample_layout(Hm, Wm, z, h, w, p, b):
    g = torch.Generator().manual_seed(41)
    mom = torch.cat([2 * torch.randn((2, Hm, Wm, z), generator=g), 3 * torch.randn((2, Hm, Wm, z), generator=g) - 2], -1).to(BF16)
    noise = torch.randn((2, z, Hm, Wm), generator=g).to(BF16)
    # one of the two log-variances on an exp tie (-0.449) lies where 3N - 2 is dense: a draw that hits one is moved to -2, so that every
    # element of every case is held to equality
    lvs = mom[..., z:]
    tie = R.exp_near_tie((0.5 * lvs.double()).to(BF16))
    lvs[tie] = -2.0
    print(f"latent sample {(Hm, Wm, z, h, w, p)} b={b}: {int(tie.sum())} of {tie.numel()} log-variances moved off an exp tie")
    assert not bool(R.exp_near_tie(torch.tensor([-1.0], dtype=BF16)).any()), "-2 itself must be no tie"
    got = _sample(mom, noise, b, h, w, p, SCALE, SHIFT)
    ref = R.latent_sample_patchify(mom, noise, b, h, w, p, SCALE, SHIFT)
    _same_bits(got, ref, f"latent sample {(Hm, Wm, z, h, w, p)} b={b}")


def test_latent_sample_rejects_a_window_larger_than_the_latent():
    lib, stream = _lib()
    mom = torch.zeros((1, 4, 4, 8), dtype=BF16, device="cuda")
    noise = torch.zeros((1, 4, 4, 4), dtype=BF16, device="cuda")
    out = Guarded(3 * 2 * 2 * 2 * 4, BF16)
    assert lib.umv_latent_sample_patchify(mom.data_ptr(), noise.data_ptr(), out.ptr(), 0, 4, 4, 4, 3, 2, 2, 1.0, 0.0, stream()) != 0
    assert lib.umv_latent_sample_patchify(mom.data_ptr(), noise.data_ptr(), out.ptr(), 0, 4, 4, 4, 2, 3, 2, 1.0, 0.0, stream()) != 0
    assert out.untouched()


# ----------------------------------------------------------------------------- the shift constant on the device
def test_device_torch_keeps_the_shift_in_fp32():
    """the reference model runs on a device, where torch hands the Python scalar of `bf16_tensor +- scalar` to the kernel as fp32 (on the
    CPU it is rounded to bf16 first, test_vae_ref_cpu.py): the two bf16 expressions of the reference, evaluated by torch on the device
    over every finite bf16 value, equal the models - and so the kernels, which the tests above hold to the models bit for bit"""
    _lib()
    v = R.all_bf16()
    v = v[torch.isfinite(v.float())]
    vd = v.cuda()
    dec = (vd / SCALE + SHIFT).cpu()
    enc = (SCALE * (vd - SHIFT)).cpu()
    _same_bits(dec, R.add_c(R.div_c(v, SCALE), SHIFT).to(BF16), "v / scale + shift on the device")
    _same_bits(enc, R.mul_c(R.sub_c(v, SHIFT), SCALE).to(BF16), "scale * (v - shift) on the device")


# ----------------------------------------------------------------------------- umv_groupnorm_nhwc_bf16
GN_SHAPES = [(32, 1), (32, 255), (64, 256), (96, 257), (160, 2307), (2048, 3), (512, 1024)]


def _gn_inputs(C, HW):
    d = _randn((HW, C), 51) * 2
    x = torch.stack([d, 3 * d + 8.0]).to(BF16)                            # sample 1: sample 0's draw times 3, moved by 4 of its deviations
    return x, (_randn((C,), 52) + 1).to(BF16), _randn((C,), 53).to(BF16)


def _groupnorm(x, gamma, beta, swish):
    lib, stream = _lib()
    B, HW, C = x.shape
    out = Guarded(B * HW * C, BF16)
    ws = torch.empty(lib.umv_groupnorm_workspace_bytes(B, HW) // 4 + 16, dtype=torch.float32, device="cuda")
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    rc = lib.umv_groupnorm_nhwc_bf16(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), out.ptr(), ws.data_ptr(), B, HW, C, 1e-6, swish, stream())
    return rc, out


@pytest.mark.parametrize("C,HW", GN_SHAPES)
def test_groupnorm_against_fp64(C, HW):
    """C = 96 / 160: the partial sums' octet-to-thread maps that do not divide 256 and the rounded-up apply grid; 2307 pixels: 10 chunks
    over 8 finalize lanes.  Every element is the model's bf16 value or its neighbour, except where the value is a cancellation so deep
    that the fp32 chain's own error (vae_ref.groupnorm_fp32_allowance: 3.25 * 2^-20 of the terms, derived there) exceeds the result's
    ulp: such an element may be that allowance, plus the rounding of the result (one ulp), from the model."""
    x, gamma, beta = _gn_inputs(C, HW)
    rc, out = _groupnorm(x, gamma, beta, 0)
    assert rc == 0
    got = out.fetch()[0].view(2, HW, C)
    ref = R.groupnorm(x, gamma, beta, 1e-6, False)
    allow = R.groupnorm_fp32_allowance(x, gamma, beta, 1e-6)
    st = R.steps(got, ref)
    d = (got.double() - ref.double()).abs()
    far = st > 1
    exact = float((st == 0).float().mean())
    print(f"groupnorm C={C} HW={HW}: {100 * exact:.3f} % bit-equal, {int((st == 1).sum())} neighbours, {int(far.sum())} more than one bf16 "
          f"value off" + (f", the worst of those {float((d / allow)[far].max()):.2f} of the fp32 allowance" if bool(far.any()) else ""))
    assert bool(torch.isfinite(got.float()).all())
    bad = far & (d > allow + R.bf16_ulp(ref.double()))
    assert not bool(bad.any()), f"{int(bad.sum())} values beyond one bf16 value and beyond the fp32 chain's allowance"
    assert exact >= 0.99
    if HW == 1 and C == 32:
        _same_bits(got, beta.expand(2, 1, C).contiguous(), "one value per group normalises to beta")


@pytest.mark.parametrize("C,HW", GN_SHAPES)
def test_groupnorm_swish_is_the_chain_on_its_own_output(C, HW):
    x, gamma, beta = _gn_inputs(C, HW)
    rc0, out0 = _groupnorm(x, gamma, beta, 0)
    rc1, out1 = _groupnorm(x, gamma, beta, 1)
    assert rc0 == 0 and rc1 == 0
    _same_bits(out1.fetch()[0], R.swish_chain(out0.fetch()[0]), f"swish C={C} HW={HW}")


def test_groupnorm_rejects_a_width_that_is_no_multiple_of_32():
    x, gamma, beta = _gn_inputs(48, 4)
    rc, out = _groupnorm(x, gamma, beta, 0)
    assert rc != 0 and out.untouched()


# ----------------------------------------------------------------------------- umv_softmax_rows_f32
@pytest.mark.parametrize("all_inf_row", [False, True])
@pytest.mark.parametrize("n", [2, 510, 512, 514, 8190, 8192, 8194])
def test_softmax_rows(n, all_inf_row):
    lib, stream = _lib()
    rows, ld = 3, n + 6
    S = torch.full((rows, ld), 1e30)                                       # the slack columns would win every maximum if read
    S[:, :n] = _randn((rows, n), 61) * 5
    if n > 2:
        S[1, torch.arange(0, n, 7)] = float("-inf")
    S[1, n - 1] = float("-inf")
    if all_inf_row:
        S[2, :n] = float("-inf")
    P, l = Guarded(rows * ld, BF16), Guarded(rows, torch.float32)
    Sd = S.cuda()
    assert lib.umv_softmax_rows_f32(Sd.data_ptr(), ld, P.ptr(), ld, l.ptr(), rows, n, 0.5, stream()) == 0
    (got, raw), lg = P.fetch(), l.fetch()[0].double()
    got, raw = got.view(rows, ld), raw.view(rows, ld)
    assert bool((raw[:, n:] == P.pat).all()), "the slack columns of P were written"
    got = got[:, :n]
    Pe, le = R.softmax_rows(S[:, :n], 0.5)
    ref = R.rbf(Pe).to(BF16)
    st = R.steps(got, ref)
    exact = float((st == 0).float().mean())
    print(f"softmax n={n}: {100 * exact:.3f} % bit-equal, {int((st == 1).sum())} neighbours, max |l / sum - 1| "
          f"{float(((lg - le).abs() / le.clamp_min(1e-300)).max()):.2e}")
    assert not bool(torch.isnan(got.float()).any()) and not bool(torch.isnan(lg).any())
    assert bool((st <= 1).all()), f"{int((st > 1).sum())} weights more than one bf16 value from the model"
    assert exact >= 0.99
    live = torch.isfinite(S[:, :n]).any(-1)
    at_max = S[:, :n] == S[:, :n].max(-1, keepdim=True).values
    assert bool((got.float()[at_max & live[:, None]] == 1.0).all())
    assert bool((R.bits(got)[torch.isinf(S[:, :n])] == 0).all()), "a -inf score must weigh exactly +0"
    assert bool(((lg - le).abs() <= 1e-5 * le).all())
    if all_inf_row:
        assert not bool(live[2]) and float(lg[2]) == 0.0 and bool((R.bits(got[2]) == 0).all())


# ----------------------------------------------------------------------------- umv_rowscale_f32_bf16
@pytest.mark.parametrize("rows,C", [(3, 2), (5, 510), (257, 6)])
def test_rowscale(rows, C):
    lib, stream = _lib()
    ld = C + 2
    O = torch.full((rows, ld), 1e30)
    O[:, :C] = _randn((rows, C), 71) * 40
    l = torch.rand(rows, generator=torch.Generator().manual_seed(72)) * 300 + 1
    l[1], l[2] = 0.0, -2.5
    out = Guarded(rows * ld, BF16)
    Od, ld_ = O.cuda(), l.cuda()
    assert lib.umv_rowscale_f32_bf16(Od.data_ptr(), ld, ld_.data_ptr(), out.ptr(), ld, rows, C, stream()) == 0
    got, raw = out.fetch()
    got, raw = got.view(rows, ld), raw.view(rows, ld)
    assert bool((raw[:, C:] == out.pat).all()), "the slack columns were written"
    got = got[:, :C]
    ref = R.rbf(R.rowscale(O[:, :C], l)).to(BF16)
    st = R.steps(got, ref)
    exact = float((st == 0).float().mean())
    print(f"rowscale {rows} x {C}: {100 * exact:.3f} % bit-equal, {int((st == 1).sum())} neighbours")
    assert bool((st <= 1).all()) and exact >= 0.999
    assert bool((got[1:3].float() == 0).all()), "rows with l <= 0 are zero"


def test_rowscale_rejects_an_odd_width():
    lib, stream = _lib()
    O = torch.zeros((2, 6), device="cuda")
    l = torch.ones(2, device="cuda")
    out = Guarded(12, BF16)
    assert lib.umv_rowscale_f32_bf16(O.data_ptr(), 6, l.data_ptr(), out.ptr(), 6, 2, 5, stream()) != 0
    assert out.untouched()
