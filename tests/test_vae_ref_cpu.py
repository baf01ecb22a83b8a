"""The reference models of tests/vae_ref.py themselves, against torch on the CPU, over every bf16 value where the chain is
scalar.  Also pins the one place where torch-CPU and the kernels' arithmetic differ: the VAE's shift_factor.  torch on the CPU
rounds the Python scalar of `bf16_tensor +- scalar` to bf16 (0.1159 -> 0.11572265625) and keeps it in fp32 for * and /; the kernels
(and torch on a device) keep fp32 throughout.  So oracle/unimedvl_cpu.py's vae_encode / vae_decode and the goldens differ from the
kernels by at most one bf16 ulp at those two steps.
conv2d, the model of the convolutions, is held to a loop nest and to the oracle's convolution, and the exact-grid inputs of
tests/conv_cases.py to the conditions that make equality of bits the contract of tests/test_vae_conv_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

import conv_cases as CC
import vae_ref as R

BF16 = torch.bfloat16
SCALE, SHIFT = 0.3611, 0.1159
SHIFT_BF16 = float(torch.tensor(SHIFT).bfloat16())


def _finite():
    v = R.all_bf16()
    return v[torch.isfinite(v.float())]


def test_pixels_u8_equals_torch_on_every_bf16_value():
    v = R.all_bf16()
    v = v[~torch.isnan(v.float())]
    ref = ((v * 0.5 + 0.5).clamp(0, 1) * 255).to(torch.uint8)
    got = R.pixels_u8(v)
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {v.numel()} values differ"
    assert torch.unique(got).numel() == 256, "every output level must occur"


def test_swish_chain_equals_torch_on_every_finite_bf16_value():
    v = _finite()
    assert torch.equal(R.bits(R.swish_chain(v)), R.bits(v * torch.sigmoid(v)))


def test_division_and_multiplication_steps_equal_torch():
    v = _finite()
    assert v.numel() == 65280
    for c in (SCALE, 1.5305, 1.0):
        assert torch.equal(R.bits(R.div_c(v, c).to(BF16)), R.bits(v / c)), f"v / {c}"
        assert torch.equal(R.bits(R.mul_c(v, c).to(BF16)), R.bits(c * v)), f"{c} * v"


def _ulp_of_largest(a, r1, r2):
    """one bf16 ulp of the largest of |a|, |shift| and the two results of a +- shift.  The two shifts differ by 1.8e-4, less than half
    a bf16 ulp of the shift (4.9e-4), so the two exact sums round to the same or to neighbouring points of the RESULT's grid; that grid
    is the larger operand's, or one binade up when the sum carries (0.0096 + 0.1159 -> 0.125 / 0.1259765625), and finer when it cancels"""
    m = torch.maximum(torch.maximum(a.abs(), torch.tensor(SHIFT, dtype=torch.float64)), torch.maximum(r1.abs(), r2.abs()))
    return R.bf16_ulp(m)


def _unpatchify_flat(v, shift):
    return R.unpatchify_latent(v.float().view(1, -1), 1, 1, 1, v.numel(), SCALE, shift).view(-1)


def test_unpatchify_shift_rounded_to_bf16_is_torch_cpu():
    """oracle/unimedvl_cpu.py vae_decode: z.to(bf16) / scale_factor + shift_factor, on every finite bf16 value"""
    v = _finite()
    ref = v / SCALE + SHIFT
    got = _unpatchify_flat(v, SHIFT_BF16)
    assert torch.equal(R.bits(got), R.bits(ref)), f"{int((R.bits(got) != R.bits(ref)).sum())} values differ"


def test_unpatchify_fp32_shift_within_one_ulp_of_torch_cpu():
    v = _finite()
    ref = (v / SCALE + SHIFT).double()
    got = _unpatchify_flat(v, SHIFT).double()
    a = (v / SCALE).double()
    ok = torch.isfinite(ref) & torch.isfinite(got)
    assert torch.equal(torch.isfinite(ref), torch.isfinite(got))
    ulp = _ulp_of_largest(a, ref, got)
    d = (got - ref).abs()
    n = int((d[ok] != 0).sum())
    print(f"unpatchify chain, fp32 shift against torch-CPU: {n} of {int(ok.sum())} finite results differ, "
          f"worst {float((d / ulp)[ok].max()):.3g} ulp")
    assert n > 0, "the fp32 constant must be visible: torch-CPU rounds it to bf16"
    assert bool((d[ok] <= ulp[ok]).all())


def _triples(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    mean = (2 * torch.randn(n, generator=g)).to(BF16)
    logvar = (3 * torch.randn(n, generator=g) - 2).to(BF16)
    noise = torch.randn(n, generator=g).to(BF16)
    return mean, logvar, noise


def _sample_flat(mean, logvar, noise, scale, shift):
    n = mean.numel()
    mom = torch.cat([mean, logvar]).view(1, 1, 2, n).permute(0, 1, 3, 2).contiguous()     # [1, 1, n, 2]: z = 1, Wm = n
    return R.latent_sample_patchify(mom, noise.view(1, 1, 1, n), 0, 1, n, 1, scale, shift).view(-1)


def test_latent_sample_shift_rounded_to_bf16_is_torch_cpu():
    """oracle/unimedvl_cpu.py vae_encode on 2^20 random (mean, logvar, noise).  torch's expf is correct to 1 fp32 ulp, so the (at most
    two, next test) half-log-variances that exp_near_tie flags are left out of the comparison"""
    mean, logvar, noise = _triples(1 << 20)
    ref = SCALE * ((mean + torch.exp(0.5 * logvar) * noise) - SHIFT)
    got = _sample_flat(mean, logvar, noise, SCALE, SHIFT_BF16)
    tie = R.exp_near_tie(0.5 * logvar)
    ne = (R.bits(got) != R.bits(ref)) & ~tie
    print(f"encoder tail, bf16 shift against torch-CPU: {int(ne.sum())} differ, {int(tie.sum())} of {tie.numel()} left out as exp ties")
    assert tie.float().mean().item() < 1e-3
    assert not bool(ne.any()), f"{int(ne.sum())} triples differ"


def test_latent_sample_fp32_shift_within_one_ulp_of_torch_cpu():
    """with scale = 1 the last product is exact, so the result is the subtraction's"""
    mean, logvar, noise = _triples(1 << 20)
    zz = mean + torch.exp(0.5 * logvar) * noise
    ref = (1.0 * (zz - SHIFT)).double()
    got = _sample_flat(mean, logvar, noise, 1.0, SHIFT).double()
    ok = ~R.exp_near_tie(0.5 * logvar) & torch.isfinite(ref)
    ulp = _ulp_of_largest(zz.double(), ref, got)
    d = (got - ref).abs()
    share = float((d[ok] != 0).float().mean())
    rel = float((d / ref.abs())[ok & (ref != 0) & (got != 0)].max())
    print(f"encoder tail, fp32 shift against torch-CPU: {100 * share:.2f} % differ, worst relative difference {rel:.3g}")
    assert share > 0
    assert bool((d[ok] <= ulp[ok]).all())


def test_exp_near_tie_flags_at_most_two_half_log_variances():
    """the cap that keeps the exemption of the GPU test from hiding anything"""
    lv = _finite()
    x = torch.unique(R.bits(0.5 * lv)).view(BF16)
    e = torch.exp(x.double())
    live = x[torch.isfinite(e) & (e > 0)]
    n2, n4 = int(R.exp_near_tie(live, 2).sum()), int(R.exp_near_tie(live, 4).sum())
    print(f"exp ties among {live.numel()} half-log-variances with a finite non-zero exp: {n2} within 2 fp32 ulps, {n4} within 4")
    assert n2 <= 2
    assert not bool(R.exp_near_tie(torch.zeros(1, dtype=BF16)).any())                    # exp(0) = 1 is a bf16 value, no tie


# ----------------------------------------------------------------------------- conv2d: the model of umv_conv2d_nhwc_bf16
def _conv_loops(x, w, bias, res, mode):
    """the convolution as a loop nest over output pixel and filter tap, with the index arithmetic of each mode written out"""
    Cout, Cin, ks, _ = w.shape
    B, Hin, Win, _ = x.shape
    x64, w64 = x.double(), w.double()
    if mode == 0:
        Hout, Wout, pad = Hin, Win, (ks - 1) // 2
    elif mode == 1:
        Hout, Wout = 2 * Hin, 2 * Win
    else:
        Hout, Wout = len(range(0, Hin + 1 - 2, 2)), len(range(0, Win + 1 - 2, 2))     # top-left corners 0, 2, .. of a 3-wide window in n + 1
    out = torch.zeros((B, Hout, Wout, Cout), dtype=BF16)
    for b in range(B):
        for oy in range(Hout):
            for ox in range(Wout):
                acc = torch.zeros(Cout, dtype=torch.float64)
                for ky in range(ks):
                    for kx in range(ks):
                        if mode == 0:
                            iy, ix = oy + ky - pad, ox + kx - pad
                            inside = 0 <= iy < Hin and 0 <= ix < Win
                        elif mode == 1:
                            uy, ux = oy + ky - 1, ox + kx - 1                       # in the upsampled image
                            inside = 0 <= uy < 2 * Hin and 0 <= ux < 2 * Win
                            iy, ix = uy >> 1, ux >> 1
                        else:
                            iy, ix = 2 * oy + ky, 2 * ox + kx                       # the pad is on the bottom and the right only
                            inside = iy < Hin and ix < Win
                        if inside:
                            acc += w64[:, :, ky, kx] @ x64[b, iy, ix]
                v = R.rbf(acc + (bias.double() if bias is not None else 0.0))
                if res is not None:
                    v = R.rbf(v + res[b, oy, ox].double())
                out[b, oy, ox] = v.to(BF16)
    return out


def _small_case(ks, mode, Cin, Cout, B, Hin, Win, flags, i):
    return CC.Case(ks, mode, Cin, Cout, B, Hin, Win, "b" in flags, "r" in flags, 900 + i, *CC._SCALES[i % len(CC._SCALES)])


_LOOP_CASES = [(3, 0, 8, 5, 2, 3, 4, "br"), (1, 0, 8, 3, 1, 2, 3, "b"), (3, 0, 16, 4, 1, 1, 1, "r"),
               (3, 1, 8, 4, 2, 1, 1, "b"), (3, 1, 8, 3, 1, 2, 3, "br"), (3, 1, 16, 2, 1, 3, 2, ""),
               (3, 2, 8, 4, 2, 2, 2, "b"), (3, 2, 8, 3, 1, 3, 5, "br"), (3, 2, 16, 2, 1, 5, 4, ""), (3, 2, 8, 2, 1, 4, 1, "b")]


@pytest.mark.parametrize("i", range(len(_LOOP_CASES)))
def test_conv2d_equals_a_loop_nest(i):
    c = _small_case(*_LOOP_CASES[i], i)
    x, w, bias, res, _ = CC.make_inputs(c)
    got = R.conv2d(x, w, bias, res, c.mode)
    ref = _conv_loops(x, w, bias, res, c.mode)
    assert got.shape == ref.shape and got.dtype == BF16
    assert bool((R.steps(got, ref) == 0).all())
    if got.numel():
        assert bool((got.float() != 0).any())


def _oracle_conv(x, w, bias, res, mode, ks):
    """the convolution as oracle/unimedvl_cpu.py has it: OracleBagel._conv (F.conv2d on bf16 tensors) called as the oracle's vae_encoder,
    vae_decode and _resblock call it - F.interpolate(scale_factor=2.0, mode="nearest") before it for the upsample, F.pad(h, (0, 1, 0, 1))
    and stride 2 without padding for the downsample, padding 0 for a 1 x 1, and the residual as a bf16 `x + h`"""
    from types import SimpleNamespace
    from oracle.unimedvl_cpu import OracleBagel
    o = SimpleNamespace(vae_sd={"c.weight": w, "c.bias": bias})
    h = x.permute(0, 3, 1, 2).contiguous()
    if mode == 0:
        y = OracleBagel._conv(o, h, "c", padding=(ks - 1) // 2)
    elif mode == 1:
        y = OracleBagel._conv(o, F.interpolate(h, scale_factor=2.0, mode="nearest"), "c")
    else:
        y = OracleBagel._conv(o, F.pad(h, (0, 1, 0, 1), mode="constant", value=0), "c", stride=2, padding=0)
    y = y.permute(0, 2, 3, 1).contiguous()
    return y if res is None else res + y


_ORACLE_CASES = [c for c in CC.CASES if c.B * c.Hin * c.Win <= 1024]


@pytest.mark.parametrize("c", _ORACLE_CASES, ids=CC.case_id)
def test_conv2d_equals_the_oracle_on_grid_inputs(c):
    """torch accumulates a bf16 convolution in fp32 and rounds once after the bias; on grid inputs every fp32 order is exact, so the
    oracle's conv, upsample and downsample equal the model bit for bit"""
    x, w, bias, res, _ = CC.make_inputs(c)
    got = R.conv2d(x, w, bias, res, c.mode)
    ref = _oracle_conv(x, w, bias, res, c.mode, c.ks)
    assert got.shape == ref.shape and ref.dtype == BF16
    ne = R.steps(got, ref) != 0
    assert not bool(ne.any()), f"{int(ne.sum())} of {ne.numel()} differ"


@pytest.mark.parametrize("c", CC.CASES, ids=CC.case_id)
def test_conv_case_inputs_meet_their_conditions(c):
    """what makes bit equality the contract of tests/test_vae_conv_gpu.py, per case of the table: conditions on the data, not measurements"""
    x, w, bias, res, unit = CC.make_inputs(c)
    out, pre1, pre2 = R.conv2d_parts(x, w, bias, res, c.mode)
    # exactness: the largest count of grid units any summation order can reach stays two bits below fp32's 24
    worst = R.conv2d_parts(x.abs(), w.abs(), None, None, c.mode)[1]
    worst = worst + (bias.double().abs() if bias is not None else 0.0) + (res.double().abs() if res is not None else 0.0)
    counts = worst / unit
    assert bool((counts == counts.round()).all()), "every term is a whole number of grid units"
    assert float(counts.max()) < 2.0 ** 22, f"sum |x||w| + |b| + |res| reaches {float(counts.max()):.3g} units"
    # the roundings are exercised: inexact sums, exact ties, and something to compare
    inexact, tie = R.bf16_inexact(pre1), R.bf16_tie(pre1)
    if pre2 is not None:
        inexact, tie = inexact | R.bf16_inexact(pre2), tie | R.bf16_tie(pre2)
    share = float(inexact.double().mean())
    print(f"{CC.case_id(c)}: {100 * share:.0f} % of {out.numel()} outputs need rounding, {100 * float(tie.double().mean()):.0f} % are ties")
    assert share >= 0.20 if c.ks == 3 else share > 0
    assert int(tie.sum()) >= 1
    assert bool((out.float() != 0).any())
    if pre2 is not None:
        assert bool((R.rbf(pre1 + res.double()) != R.rbf(R.rbf(pre1) + res.double())).any()), "dropping the first rounding must show"


def test_conv_table_holds_the_cases_of_each_kernel():
    assert len(CC.CASES) == 31 and len(set(CC.CASES)) == 31
    for group in (CC.GATHER_16x256 + CC.GATHER_128x64 + CC.GATHER_128x128, CC.PATCH_0, CC.PATCH_1):
        assert any(not c.bias for c in group) and any(c.bias for c in group) and any(c.res for c in group)
    assert all(c.Cout <= 16 for c in CC.GATHER_16x256) and all(c.Cout > 16 for c in CC.GATHER_128x64)
    assert all(CC.patch_ok(c.ks, c.mode, c.Cin, c.Cout) and c.mode == m for m, grp in ((0, CC.PATCH_0), (1, CC.PATCH_1)) for c in grp)
    assert any(c.mode == 1 and c.res for c in CC.CASES)
    (big,) = CC.GATHER_128x128
    wg = lambda B: ((B * big.Hin * big.Win + 127) // 128) * ((big.Cout + 127) // 128)
    assert wg(2) >= 384 > wg(1), "the one shape whose tile depends on the batch"


def test_conv2d_downsample_of_one_row_or_column_is_empty():
    """a 3 x 3 stride-2 window has no place in the 2 rows that F.pad(0, 1, 0, 1) makes of one: vae.py's floor division gives 0 rows"""
    x = torch.ones((1, 1, 3, 8), dtype=BF16)
    w = torch.ones((8, 8, 3, 3), dtype=BF16)
    assert R.conv2d_out_hw(1, 3, 3, 2) == (0, 1) and R.conv2d_out_hw(3, 1, 3, 2) == (1, 0) and R.conv2d_out_hw(2, 3, 3, 2) == (1, 1)
    assert tuple(R.conv2d(x, w, None, None, 2).shape) == (1, 0, 1, 8)
    assert tuple(R.conv2d(x.permute(0, 2, 1, 3), w, None, None, 2).shape) == (1, 1, 0, 8)
    with pytest.raises(RuntimeError):
        F.conv2d(F.pad(x.permute(0, 3, 1, 2).float(), (0, 1, 0, 1)), w.float(), stride=2)


def test_normal_bf16_draw_and_one_hot_weight():
    v = CC.normal_bf16_draw(2 * 17 * 15 * 64, 7)
    f = v.double()
    assert bool(torch.isfinite(f).all()) and bool(((f == 0) | (f.abs() >= 2.0 ** -126)).all())
    assert torch.unique(R.bits(v)).numel() == v.numel()
    assert torch.unique((R.bits(v).to(torch.int32) >> 7) & 0xFF).numel() >= 254          # every exponent of a normal value
    w = CC.one_hot_weight(8, 5)
    assert float(w.sum()) == 8 and bool((w[:, :, 1, 2] == torch.eye(8)).all())
