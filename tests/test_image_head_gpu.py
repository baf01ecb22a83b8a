"""umv_cfg_renorm_euler (csrc/image_head.hip) through ops.cfg_renorm_euler, against a torch CPU restatement in bf16 of the
guidance + renorm of oracle/unimedvl_cpu.py:481-500 followed by the Euler step `x_t -= v * dt` with x_t in fp32.

Two segments of 3 and of 40 tokens (one smaller than a workgroup; the other needs the strided loops and has more tokens than the
workgroup has waves), `rows` a permutation into velocity buffers with a row stride of D + 8."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SEGS = (3, 40)
DT, S_TEXT = 1.0 / 24.0, 4.0
RTYPES = {"global": 0, "channel": 1, "text_channel": 2}


@functools.lru_cache(maxsize=None)
def inputs(D):
    """(x_t fp32 [N, D], the three velocity buffers bf16 [N, D + 8], rows int32 [N]); shared by every case, never written to"""
    g = torch.Generator().manual_seed(100 + D)
    N = sum(SEGS)
    x_t = torch.randn(N, D, generator=g)
    bufs = tuple(torch.randn(N, D + 8, generator=g).to(BF16) for _ in range(3))
    rows = torch.randperm(N, generator=g).to(torch.int32)
    return x_t, bufs, rows


def guided_velocity(v_t, v_c, v_i, cfg_text_scale, cfg_img_scale, cfg_renorm_min, cfg_renorm_type):
    """oracle/unimedvl_cpu.py:481-500 on the bf16 tensors of ONE sample (the reference is batch-1: "global" norms are per sample)"""
    if cfg_text_scale > 1.0:
        if cfg_renorm_type == "text_channel":
            v_text_ = v_c + cfg_text_scale * (v_t - v_c)
            n0 = torch.norm(v_t, dim=-1, keepdim=True)
            n1 = torch.norm(v_text_, dim=-1, keepdim=True)
            scale = (n0 / (n1 + 1e-8)).clamp(min=cfg_renorm_min, max=1.0)
            v_text = v_text_ * scale
            v_t = v_i + cfg_img_scale * (v_text - v_i) if cfg_img_scale > 1.0 else v_text
        else:
            v_text_ = v_c + cfg_text_scale * (v_t - v_c)
            v_ = v_i + cfg_img_scale * (v_text_ - v_i) if cfg_img_scale > 1.0 else v_text_
            if cfg_renorm_type == "global":
                n0, n1 = torch.norm(v_t), torch.norm(v_)
            else:
                n0 = torch.norm(v_t, dim=-1, keepdim=True)
                n1 = torch.norm(v_, dim=-1, keepdim=True)
            scale = (n0 / (n1 + 1e-8)).clamp(min=cfg_renorm_min, max=1.0)
            v_t = v_ * scale
    return v_t


@functools.lru_cache(maxsize=None)
def reference(D, s_text, s_img, renorm_min, rtype):
    """(x_t after the step, max |v * dt|), segment by segment as the kernel does"""
    x_t, (bt, bc, bi), rows = inputs(D)
    r = rows.long()
    v_t, v_c, v_i = bt[r, :D], bc[r, :D], bi[r, :D]
    out, step_max, n0 = x_t.clone(), 0.0, 0
    for n in SEGS:
        s = slice(n0, n0 + n)
        v = guided_velocity(v_t[s], v_c[s], v_i[s], s_text, s_img, renorm_min, rtype)
        assert v.dtype == BF16
        step = v * DT                      # bf16
        out[s] -= step                     # fp32
        step_max = max(step_max, step.float().abs().max().item())
        n0 += n
    return out, step_max


def run_kernel(D, s_text, s_img, renorm_min, rtype):
    from unimedvl_amd import ops
    x_t, (bt, bc, bi), rows = inputs(D)
    x = x_t.cuda()
    seg_off = torch.tensor([0, SEGS[0], sum(SEGS)], dtype=torch.int32).cuda()
    v_text = bc.cuda() if s_text > 1.0 else None
    v_img = bi.cuda() if (s_text > 1.0 and s_img > 1.0) else None
    ops.cfg_renorm_euler(x, bt.cuda(), v_text, v_img, rows.cuda(), seg_off, len(SEGS), s_text, s_img, renorm_min,
                         RTYPES[rtype], DT)
    torch.cuda.synchronize()
    return x.cpu()


GRID = [(D, s_img, rtype) for D in (64, 96) for s_img in (1.0, 1.5) for rtype in RTYPES]


@pytest.mark.parametrize("D,s_img,rtype", GRID)
def test_unit_scale_is_bit_exact(D, s_img, rtype):
    """renorm_min = 1.0: the scale is exactly 1 and every remaining operation is elementwise with the reference's roundings"""
    ref, _ = reference(D, S_TEXT, s_img, 1.0, rtype)
    got = run_kernel(D, S_TEXT, s_img, 1.0, rtype)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), f"{int((got != ref).sum())} of {got.numel()} elements differ"


@pytest.mark.parametrize("D", [64, 96])
def test_no_guidance_is_bit_exact(D):
    ref, _ = reference(D, 1.0, 1.0, 0.0, "global")
    got = run_kernel(D, 1.0, 1.0, 0.0, "global")
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), f"{int((got != ref).sum())} of {got.numel()} elements differ"


@pytest.mark.parametrize("D,s_img,rtype", GRID)
def test_renorm_within_three_ulps_of_the_step(D, s_img, rtype):
    """renorm_min = 0.0: the kernel's fp32 sums run in another order than torch's, so the bf16 scale may differ by one ulp.  Three
    bf16 ulps of the largest step: one from the scale, one from each of the two roundings after it."""
    ref, step_max = reference(D, S_TEXT, s_img, 0.0, rtype)
    got = run_kernel(D, S_TEXT, s_img, 0.0, rtype)
    err = (got - ref).abs().max().item()
    print(f"D={D} s_img={s_img} {rtype}: max err {err:.3e}, bound {3 * 2 ** -8 * step_max:.3e}, "
          f"{100 * (got == ref).float().mean().item():.2f}% of the elements match exactly")
    assert err <= 3 * 2 ** -8 * step_max, f"max err {err} > {3 * 2 ** -8 * step_max}"
