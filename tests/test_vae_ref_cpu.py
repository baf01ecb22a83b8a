"""The reference models of tests/vae_ref.py themselves, against torch on the CPU, over every bf16 value where the chain is
scalar.  Also pins the one place where torch-CPU and the kernels' arithmetic differ: the VAE's shift_factor.  torch on the CPU
rounds the Python scalar of `bf16_tensor +- scalar` to bf16 (0.1159 -> 0.11572265625) and keeps it in fp32 for * and /; the kernels
(and torch on a device) keep fp32 throughout.  So oracle/unimedvl_cpu.py's vae_encode / vae_decode and the goldens differ from the
kernels by at most one bf16 ulp at those two steps."""
import torch

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
