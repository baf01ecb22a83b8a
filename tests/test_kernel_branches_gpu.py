"""Every dispatch branch of the two MFMA-bound kernel families, at the shapes the headline bench runs, against an fp32
reference of the same op (VERDICT r01 "missing" #1 / "next" #2).

The tiny-model goldens only reach the 128x64 GEMM tile and the TQ = 1 attention kernels; the variants that carry the
bench - gemm_tiled_kernel<2,4,8,4,1,4,1> (cfg 266: hand-interleaved 256x256x32), <4,2,...,1> (268), <2,2,...,1> (270) and
attn_prefill_kernel<128|72, 2> (two q-tiles per wave, hand-placed MFMA wait states) - are pinned here:
  * the shape -> kernel policy is asserted through the host-only queries umv_gemm_tile_config / umv_attn_prefill_tq,
    so a policy change cannot silently move these cases onto another kernel;
  * GEMM reference: torch fp32 matmul on the same device (fp32 accumulate, rounded once to bf16 like the kernel);
  * attention reference: fp32 scores / softmax, P rounded to bf16 before PV (the flash-attn model the oracle uses,
    oracle/unimedvl_cpu.py::attention_segment impl="flash"), evaluated in fp32 on the device;
  * tools/attn_ab.py's sha compare (per-wave kernel == LDS-shared TQ=1 == TQ=2, bit for bit) runs as a test.
Reference call sites: qwen2_navit.py:605-614, siglip_navit.py:232-241 (attention); every nn.Linear of the LLM / ViT.
"""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd import ops as o
    return o


def _lib():
    from unimedvl_amd import _lib
    return _lib.load()


def ulp_diff(a, b):
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
        return torch.where(i >= 0x8000, 0x8000 - i, i)
    return (key(a) - key(b)).abs()


def check_bf16(got, ref, max_ulp, frac_exact, what, mag=None, two_roundings=False):
    """got / ref bf16 on the device: no element further than max_ulp (unless absolutely tiny), >= frac_exact bit-exact.
    mag (optional, fp32): magnitude of the largest intermediate behind each element (a residual add can cancel: one ulp of
    the rounded GEMM result is then several ulps of the sum; or carry into the next binade) - the element passes if it is
    within max_ulp ulps OF mag."""
    assert got.shape == ref.shape
    d = ulp_diff(got, ref)
    absd = (got.float() - ref.float()).abs()
    scale = ref.float().abs().max().clamp_min(1e-6)
    bad = (d > max_ulp) & (absd > scale * 2 ** -8)
    if mag is not None:
        bad &= absd > max_ulp * 2.0 ** -7 * mag.abs()
    if two_roundings:
        # epilogues that round twice (GEMM result -> bf16, then + residual / GELU -> bf16): a one-ulp flip of the first
        # rounding (fp32 summation order at an exact tie) can land the second on a tie as well and come out 2 ulps apart
        # (tools/dbg_branch.py prints such elements with their fp64 sums); allow that for at most 1 element in 100 000
        over = bad & (d <= 2)
        assert float(over.float().mean()) <= 1e-5, f"{what}: {int(over.sum())} elements 2 ulps off"
        bad &= d > 2
    assert int(bad.sum()) == 0, f"{what}: {int(bad.sum())} elements off by more than {max_ulp} ulp; worst abs {float(absd.max()):.4g}"
    exact = (d == 0).float().mean().item()
    assert exact >= frac_exact, f"{what}: only {exact:.4f} bit-exact"
    return exact


def rnd(shape, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda") * scale).to(BF16)


def _mm(x, w):
    """fp32 reference x @ w^T in row chunks (keeps the fp32 copies small)."""
    wf = w.float()
    return torch.cat([x[i:i + 2048].float() @ wf.T for i in range(0, x.shape[0], 2048)], 0)


# (M, N, K, epilogue, expected tile config).  266: the bench's prefill shapes (8208 = 8 x 1026 image-span tokens,
# 8192 = 8 x 1024 ViT patches, 2064 = 8 flow segments of 258); 268 / 270: what short prefills and single images get.
TILED = [
    (4096, 4096, 4096, "bias", 266),
    (8208, 4608, 3584, "bias", 266),          # LLM QKV, 8 image spans
    (8208, 3584, 3584, "residual", 266),      # o_proj + residual
    (8208, 3584, 18944, "residual", 266),     # down_proj + residual
    (8208, 37888, 3584, "swiglu", 266),       # gate/up SwiGLU
    (8192, 3456, 1152, "bias", 266),          # ViT fused q/k/v
    (8192, 4304, 1152, "gelu", 384),          # ViT fc1 + GELU-tanh: 12 x 384 columns (the last block ragged)
    (8192, 1152, 4304, "residual", 288),      # ViT fc2 (+ residual): 4 x 288 columns by 64 row blocks = 256 tiles (round 3)
    (8192, 1152, 1152, "residual", 288),      # ViT out-proj
    (2048, 4608, 3584, "bias", 288),          # guided flow pass QKV (2 x 1024 latent rows): 16 x 288 columns by 16 row blocks
    (2064, 4608, 3584, "bias", 384),          # flow-pass QKV: 12 x 384 columns by 17 row blocks
    (32768, 1152, 4304, "bias", 384),         # 32 images
    (2064, 37888, 3584, "swiglu", 266),       # flow pass gate/up
    (1026, 4608, 3584, "bias", 268),          # single image span QKV
    (1026, 3584, 3584, "residual", 270),      # single image span o_proj
    (1026, 3584, 18944, "residual", 270),
    (16500, 768, 3584, "residual", 266),      # >= 16k rows: two M super-blocks (33 + 32 m-blocks), each over all n-strips
    (16500, 1280, 18944, "bias", 266),        # ... and nine of 8 (one of 1) at K = 18944
    (272, 4608, 3584, "bias", 64),            # 8 x 34 text tokens
    (300, 1152, 608, "bias", 64),             # short K (ViT patch embed, 588 padded to 608)
]


@pytest.mark.parametrize("M,N,K,epi,cfg", TILED)
def test_gemm_tiled_branch(ops, M, N, K, epi, cfg):
    lib = _lib()
    n_eff = N
    assert lib.umv_gemm_tile_config(M, n_eff, K) == cfg, f"policy moved: {M}x{N}x{K} now -> {lib.umv_gemm_tile_config(M, n_eff, K)}"
    x = rnd((M, K), 1)
    if epi == "swiglu":
        I = N // 2
        wg, wu = rnd((I, K), 2, 1 / math.sqrt(K)), rnd((I, K), 3, 1 / math.sqrt(K))
        lin = ops.PackedLinear.from_gate_up(wg, wu)
        out = ops.gemm(x, lin)
        ref = F.silu(_mm(x, wg).to(BF16)) * _mm(x, wu).to(BF16)     # modeling_qwen2.py:235, bf16 after every op
        # a 1-ulp flip of gate or up moves the product by one ulp; flips are rare (fp32 accumulation order only)
        check_bf16(out, ref, 2, 0.97, f"swiglu {M}x{N}x{K}")
        return
    w, b = rnd((N, K), 2, 1 / math.sqrt(K)), rnd((N,), 3)
    base = _mm(x, w)
    if epi == "bias":
        out = ops.gemm(x, ops.PackedLinear.from_weight(w, b))
        ref = (base + b.float()).to(BF16)
    elif epi == "gelu":
        out = ops.gemm(x, ops.PackedLinear.from_weight(w, b), act="gelu_tanh")
        ref = F.gelu((base + b.float()).to(BF16), approximate="tanh")       # siglip_navit.py:256-257
    else:
        res = rnd((M, N), 4)
        out = ops.gemm(x, ops.PackedLinear.from_weight(w), residual=res)
        ref = res + base.to(BF16)                                           # qwen2_navit.py:883,900
        mag = torch.maximum(torch.maximum(base.abs(), res.float().abs()), ref.float().abs())
        check_bf16(out, ref, 1, 0.98, f"{epi} {M}x{N}x{K}", mag=mag, two_roundings=True)
        return
    check_bf16(out, ref, 1, 0.98, f"{epi} {M}x{N}x{K}", two_roundings=(epi == "gelu"))


@pytest.mark.parametrize("M,n_text,N,K,cfg", [(2064, 16, 4608, 3584, 288), (2080, 16, 4608, 3584, 384), (8224, 16, 4608, 3584, 266), (2064, 16, 3584, 18944, 268), (1032, 8, 4608, 3584, 268)])
def test_gemm_tiled_row_indexed_mot(ops, M, n_text, N, K, cfg):
    """MoT routing at flow-pass size (qwen2_navit.py:552-562,891-898): the latent rows go through the tiled kernel by a row
    index list, the marker-token rows through the weight-streaming kernel, into one output buffer."""
    lib = _lib()
    g = torch.Generator().manual_seed(9)
    perm = torch.randperm(M, generator=g)
    text_rows, vae_rows = perm[:n_text].sort().values.to(torch.int32).cuda(), perm[n_text:].sort().values.to(torch.int32).cuda()
    assert lib.umv_gemm_tile_config(M - n_text, N, K) == cfg
    x = rnd((M, K), 11)
    wu, wg_, b = rnd((N, K), 12, 1 / math.sqrt(K)), rnd((N, K), 13, 1 / math.sqrt(K)), rnd((N,), 14)
    res = rnd((M, N), 15)
    out = res.clone()
    ops.gemm(x, ops.PackedLinear.from_weight(wu, b), out=out, M=n_text, row_idx=text_rows, residual=out)
    ops.gemm(x, ops.PackedLinear.from_weight(wg_, b), out=out, M=M - n_text, row_idx=vae_rows, residual=out)
    tl, vl = text_rows.long(), vae_rows.long()
    base = torch.empty((M, N), dtype=torch.float32, device="cuda")
    base[tl] = _mm(x[tl], wu) + b.float()
    base[vl] = _mm(x[vl], wg_) + b.float()
    ref = res + base.to(BF16)
    mag = torch.maximum(torch.maximum(base.abs(), res.float().abs()), ref.float().abs())
    check_bf16(out, ref, 1, 0.98, f"row-indexed {M}x{N}x{K}", mag=mag, two_roundings=True)


@pytest.mark.parametrize("M,N,K,swiglu", [(8, 37888, 3584, True), (8, 152064, 3584, False), (32, 37888, 3584, True),
                                          (32, 152064, 3584, False), (64, 37888, 3584, True), (48, 3584, 18944, False)])
def test_gemm_skinny_headline_shapes(ops, M, N, K, swiglu):
    """the dominant decode kernels at their real N (gate/up N = 37 888, lm_head N = 152 064) for B = 8 / 32 / 64 rows"""
    x = rnd((M, K), 21)
    if swiglu:
        wg, wu = rnd((N // 2, K), 22, 1 / math.sqrt(K)), rnd((N // 2, K), 23, 1 / math.sqrt(K))
        out = ops.gemm(x, ops.PackedLinear.from_gate_up(wg, wu))
        ref = F.silu(_mm(x, wg).to(BF16)) * _mm(x, wu).to(BF16)
        check_bf16(out, ref, 2, 0.97, f"skinny swiglu {M}x{N}x{K}")
    else:
        w = rnd((N, K), 22, 1 / math.sqrt(K))
        out = ops.gemm(x, ops.PackedLinear.from_weight(w))
        check_bf16(out, _mm(x, w).to(BF16), 1, 0.98, f"skinny {M}x{N}x{K}")


@pytest.mark.parametrize("M,N,K,S", [(8, 4608, 3584, 3), (8, 3584, 3584, 4), (8, 3584, 18944, 4), (32, 3584, 18944, 4), (64, 4608, 3584, 3)])
def test_gemm_splitk_partials_sum_to_fp32_reference(ops, M, N, K, S):
    """split-K decode mode (decode.py::_step): the fp32 partial sums of the K splits add up to x @ W^T"""
    x, w = rnd((M, K), 31), rnd((N, K), 32, 1 / math.sqrt(K))
    part = torch.empty((S, M, N), dtype=torch.float32, device="cuda")
    ops.gemm_splitk(x, ops.PackedLinear.from_weight(w), part, S)
    got = part.sum(0)
    ref = _mm(x, w)
    err = (got - ref).abs().max().item()
    assert err <= 2e-5 * math.sqrt(K) * ref.abs().max().item() + 1e-6, f"split-K fp32 sum differs by {err}"
    check_bf16(got.to(BF16), ref.to(BF16), 1, 0.98, "split-K")


@pytest.mark.parametrize("M,N,K,tile", [(300, 100, 2048, 266), (515, 1000, 1152, 268), (1000, 4300, 1152, 266), (777, 250, 1024, 270),
                                          (515, 1000, 1160, 288), (130, 300, 3584, 288),    # 288 x 128: 26 staging pieces on 8 waves
                                          (300, 100, 2048, -266), (777, 250, 1024, -270),   # negative: the half-line staging (UMV_GEMM_XLINE=0)
                                          (300, 100, 2048, 466), (1000, 4300, 1152, 466), (515, 1000, 1160, 468), (130, 300, 3584, 4384),
                                          (260, 520, 40, 466)])                             # the 4-wave AGPR tiles (gemm_w4.hip), K shorter than their prologue
def test_gemm_lds_epilogue_ragged_and_unaligned(ops, M, N, K, tile, monkeypatch):
    """The whole-row LDS epilogue of the tiled kernels (gemm_epilogue.h::epi_wave_tile_lds) on everything that leaves its 16-byte
    fast path: N not a multiple of 8 (the last 16-byte chunk of a row is partial), an output / residual row pitch that is not a
    multiple of 8 elements and a base pointer 2 bytes off 16-byte alignment (element stores, element residual loads), M with a
    ragged last tile, row-indexed scatter.  Against fp32 matmul; rows and columns outside the result must stay untouched."""
    xline = "0" if tile < 0 else "1"
    tile = abs(tile)
    monkeypatch.setenv("UMV_GEMM_TILE", str(tile))
    import subprocess as sp
    code = f"""
import sys, math, torch
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
from unimedvl_amd import ops
from test_kernel_branches_gpu import rnd, _mm, check_bf16, BF16
M, N, K = {M}, {N}, {K}
x = rnd((M, K), 1); w = rnd((N, K), 2, 1 / math.sqrt(K)); b = rnd((N,), 3)
lin = ops.PackedLinear.from_weight(w, b)
T = M + 37
pitch = N + 3                                   # odd pitch: no 8- or 16-byte aligned rows
buf = torch.full((T * pitch + 1,), 7.0, dtype=BF16, device='cuda')
out = buf[1:].view(T, pitch)[:, :N]             # base pointer 2 bytes past a 16-byte boundary
resbuf = rnd((T, N + 5), 4)
res = resbuf[:, :N]
rows = torch.randperm(T, device='cuda')[:M].sort().values.to(torch.int32)
xs = torch.zeros((T, K), dtype=BF16, device='cuda'); xs[rows.long()] = x
ops.gemm(xs, lin, out=out, M=M, row_idx=rows, residual=res)
ref = ((_mm(x, w) + b.float()).to(BF16).float() + res[rows.long()].float()).to(BF16)
check_bf16(out[rows.long()].contiguous(), ref, 1, 0.97, 'ragged lds epilogue', two_roundings=True)
keep = torch.ones(T, dtype=torch.bool, device='cuda'); keep[rows.long()] = False
assert (out[keep] == 7.0).all(), 'rows outside row_idx were written'
full = buf[1:].view(T, pitch)
assert (full[:, N:] == 7.0).all() and float(buf[0]) == 7.0, 'columns beyond N were written'
# and the plain (dense, aligned-base) form with a GELU epilogue on the same ragged N
o2 = ops.gemm(x, lin, act='gelu_tanh')
r2 = torch.nn.functional.gelu((_mm(x, w) + b.float()).to(BF16), approximate='tanh')
check_bf16(o2, r2, 1, 0.97, 'ragged gelu', two_roundings=True)
print('OK')
"""
    r = sp.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, UMV_GEMM_TILE=str(tile), UMV_GEMM_XLINE=xline))
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


@pytest.mark.parametrize("tile", [266, 268, 384, 270])
def test_full_line_x_staging_bit_identical(ops, tile):
    """The default staging of the interleaved tiles (gemm_tiled.h SCHED = 3: x in full 128-byte lines through an XOR-swizzled row-major
    ring, k-step pairs) against the half-line staging it replaced (UMV_GEMM_XLINE=0): the same MFMAs on the same operands in the
    same order, so every output bit must agree - full tiles, ragged M / N, K that is not a multiple of 64 or of 32 (zero-filled
    tail chunks), an odd number of k-steps, K shorter than the prologue, row-indexed A / C and the SwiGLU epilogue."""
    import subprocess as sp
    code = f"""
import hashlib, sys, math, torch
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
from unimedvl_amd import ops
from test_kernel_branches_gpu import rnd, BF16
for M, N, K in ((2048, 4608, 3584), (8192, 1152, 4304), (1000, 1152, 1160), (300, 520, 1096), (700, 3584, 96), (515, 1152, 4304), (260, 300, 40), (4099, 777, 2080)):
    x = rnd((M, K), 1); w = rnd((N, K), 2, 1 / math.sqrt(K)); b = rnd((N,), 3)
    lin = ops.PackedLinear.from_weight(w, b)
    res = rnd((M, N), 4)
    out = ops.gemm(x, lin, residual=res)
    print('sha', M, N, K, hashlib.sha256(out.cpu().view(torch.int16).numpy().tobytes()).hexdigest())
    T = M + 9
    rows = torch.randperm(T, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5))[:M].sort().values.to(torch.int32)
    xs = torch.zeros((T, K), dtype=BF16, device='cuda'); xs[rows.long()] = x
    o2 = torch.zeros((T, N), dtype=BF16, device='cuda')
    ops.gemm(xs, lin, out=o2, M=M, row_idx=rows)
    print('sha rows', M, N, K, hashlib.sha256(o2.cpu().view(torch.int16).numpy().tobytes()).hexdigest())
g, u = rnd((1024, 2048), 6, 0.02), rnd((1024, 2048), 7, 0.02)
lin = ops.PackedLinear.from_gate_up(g, u)
o3 = ops.gemm(rnd((2050, 2048), 8), lin)
print('sha swiglu', hashlib.sha256(o3.cpu().view(torch.int16).numpy().tobytes()).hexdigest())
"""
    shas = {}
    for xl in ("0", "1"):
        r = sp.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, UMV_GEMM_TILE=str(tile), UMV_GEMM_XLINE=xl))
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        shas[xl] = [ln for ln in r.stdout.splitlines() if ln.startswith("sha")]
        assert len(shas[xl]) == 17
    assert shas["0"] == shas["1"], [(a, b) for a, b in zip(shas["0"], shas["1"]) if a != b]


@pytest.mark.parametrize("tile", [266, 268, 384])
def test_gemm_w4_bit_identical(ops, tile):
    """The 4-wave tiles with the accumulators in literal AGPRs (gemm_w4.hip: 256 x 256, 256 x 128, 384 x 128; the default at every K since
    the lean epilogue; UMV_GEMM_W4=2 says so explicitly) against the 8-wave tiles of the same shape (UMV_GEMM_W4=0): the same MFMAs on
    the same operands in the same k order, so every output bit must agree - full tiles, ragged M / N, K % 64 != 0 and K % 32 != 0
    (zero-filled tail chunks), an odd number of k-steps, K shorter than the prologue, fewer k-steps than the unroll period, row-indexed
    A / C, bias + residual, bias + GELU and the SwiGLU epilogue."""
    import subprocess as sp
    code = f"""
import hashlib, sys, math, torch
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
from unimedvl_amd import ops
from test_kernel_branches_gpu import rnd, BF16
def sha(t): return hashlib.sha256(t.cpu().view(torch.int16).numpy().tobytes()).hexdigest()
for M, N, K in ((2048, 4608, 3584), (8192, 1152, 4304), (1000, 1152, 1160), (300, 520, 1096), (700, 3584, 96), (515, 1152, 4304), (260, 300, 40), (4099, 777, 2080), (130, 260, 160),
                (4500, 4616, 160), (5000, 6004, 96)):      # > 256 tiles: several rounds of tiles per CU (lean and general epilogue)
    x = rnd((M, K), 1); w = rnd((N, K), 2, 1 / math.sqrt(K)); b = rnd((N,), 3)
    lin = ops.PackedLinear.from_weight(w, b)
    res = rnd((M, N), 4)
    print('sha', M, N, K, sha(ops.gemm(x, lin, residual=res)))
    print('sha gelu', M, N, K, sha(ops.gemm(x, lin, act='gelu_tanh')))
    T = M + 9
    rows = torch.randperm(T, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5))[:M].sort().values.to(torch.int32)
    xs = torch.zeros((T, K), dtype=BF16, device='cuda'); xs[rows.long()] = x
    o2 = torch.zeros((T, N), dtype=BF16, device='cuda')
    ops.gemm(xs, lin, out=o2, M=M, row_idx=rows)
    print('sha rows', M, N, K, sha(o2))
g, u = rnd((1024, 2048), 6, 0.02), rnd((1024, 2048), 7, 0.02)
lin = ops.PackedLinear.from_gate_up(g, u)
print('sha swiglu', sha(ops.gemm(rnd((2050, 2048), 8), lin)))
"""
    shas = {}
    for w4 in ("0", "2"):
        r = sp.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, UMV_GEMM_TILE=str(tile), UMV_GEMM_W4=w4))
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        shas[w4] = [ln for ln in r.stdout.splitlines() if ln.startswith("sha")]
        assert len(shas[w4]) == 34
    assert shas["0"] == shas["2"], [(a, b) for a, b in zip(shas["0"], shas["2"]) if a != b]


_EPI_SHA_CODE = """
import hashlib, sys, math, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from unimedvl_amd import ops
from test_kernel_branches_gpu import rnd, BF16
def sha(t): return hashlib.sha256(t.cpu().view(torch.int16).numpy().tobytes()).hexdigest()
for M, N, K in ((2048, 4608, 3584), (1000, 1152, 1160), (300, 520, 1096), (700, 3584, 96), (515, 1152, 2080), (260, 300, 40), (4099, 776, 2080), (130, 264, 160)):
    x = rnd((M, K), 1); w = rnd((N, K), 2, 1 / math.sqrt(K)); b = rnd((N,), 3)
    lin, lin_nb = ops.PackedLinear.from_weight(w, b), ops.PackedLinear.from_weight(w)
    res = rnd((M, N), 4)
    print('sha plain', M, N, K, sha(ops.gemm(x, lin_nb)))
    print('sha bias', M, N, K, sha(ops.gemm(x, lin)))
    print('sha bias+res', M, N, K, sha(ops.gemm(x, lin, residual=res)))
    print('sha res', M, N, K, sha(ops.gemm(x, lin_nb, residual=res)))
    print('sha gelu', M, N, K, sha(ops.gemm(x, lin, act='gelu_tanh')))
    T = M + 9
    rows = torch.randperm(T, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5))[:M].sort().values.to(torch.int32)
    xs = torch.zeros((T, K), dtype=BF16, device='cuda'); xs[rows.long()] = x
    o2 = torch.full((T, N), 3.0, dtype=BF16, device='cuda')
    rs = rnd((T, N), 9)
    ops.gemm(xs, lin, out=o2, M=M, row_idx=rows, residual=rs)
    print('sha rows bias+res', M, N, K, sha(o2))
    o3 = torch.full((T, N + 8), 5.0, dtype=BF16, device='cuda')       # output rows wider than N: columns N.. must stay untouched
    ops.gemm(xs, lin_nb, out=o3[:, :N], M=M, row_idx=rows)
    print('sha rows pitched', M, N, K, sha(o3))
for I, K, M in ((1024, 2048, 2050), (528, 1152, 300)):
    g, u = rnd((I, K), 6, 0.02), rnd((I, K), 7, 0.02)
    lin = ops.PackedLinear.from_gate_up(g, u)
    x = rnd((M, K), 8)
    print('sha swiglu', I, K, M, sha(ops.gemm(x, lin)))
    rows = torch.arange(0, 2 * M, 2, device='cuda', dtype=torch.int32)
    xs = torch.zeros((2 * M, K), dtype=BF16, device='cuda'); xs[rows.long()] = x
    o = torch.full((2 * M, I), 2.0, dtype=BF16, device='cuda')
    ops.gemm(xs, lin, out=o, M=M, row_idx=rows)
    print('sha swiglu rows', I, K, M, sha(o))
"""


@pytest.mark.parametrize("tile,w4", [(266, 0), (268, 0), (384, 0), (270, 0), (288, 0), (64, 0), (266, 2), (268, 2), (384, 2)])
def test_gemm_lean_epilogue_bit_identical(ops, tile, w4):
    """The branch-free epilogue of the tiled GEMMs (gemm_epilogue.h::epi_wave_tile_lean: flag combination at compile time, rows beyond
    M / chunks beyond N dropped by the buffer range check, default) against the general one (UMV_GEMM_LEAN_EPI=0), on every tile
    family of the policy, 8-wave and 4-wave: plain, bias, bias + residual, residual, bias + GELU, SwiGLU, row-indexed outputs (with a
    residual; with an output pitch wider than N), ragged M and N, and shapes the lean form must decline (N % 8 != 0) - every output
    bit, including the untouched rows / columns of the destination, must agree."""
    import subprocess as sp
    code = _EPI_SHA_CODE.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    shas = {}
    for lean in ("0", "1"):
        r = sp.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900,
                   env=dict(os.environ, UMV_GEMM_TILE=str(tile), UMV_GEMM_W4=str(w4), UMV_GEMM_LEAN_EPI=lean))
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        shas[lean] = [ln for ln in r.stdout.splitlines() if ln.startswith("sha")]
        assert len(shas[lean]) == 8 * 7 + 4
    assert shas["0"] == shas["1"], [(a, b) for a, b in zip(shas["0"], shas["1"]) if a != b]


def test_skinny_full_line_x_staging_bit_identical(ops):
    """The weight-streaming kernels with x in full 128-byte lines (gemm.hip XL, the default: a k-tile pair of 8 rows per load, per-wave
    LDS staging, one piece for M <= 8, two per 16-row tile above) against the fragment-shaped loads they replaced
    (UMV_SKINNY_XL=0): same operands, same MFMAs, same order - every bit must agree.  Rows 1 .. 64, K slices that
    start on odd k-tiles (K = 3584 over 3 splits: 38 / 8 waves = 5 tiles per wave), K % 64 != 0, K % 32 != 0, split-K partial sums,
    SwiGLU, residual, row-indexed x, and the e4m3 and MXFP4 images."""
    import subprocess as sp
    code = f"""
import hashlib, sys, math, torch
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
from unimedvl_amd import ops
from test_kernel_branches_gpu import rnd, BF16
def sha(t): return hashlib.sha256(t.cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32).numpy().tobytes()).hexdigest()[:16]
for N, K in ((4608, 3584), (3584, 18944), (1000, 1096), (320, 4304), (96, 96)):
    w = rnd((N, K), 2, 1 / math.sqrt(K)); b = rnd((N,), 3)
    for fp8 in (False, True, 'fp4'):
        if (fp8 is True and K % 64) or (fp8 == 'fp4' and K % 32):
            continue
        lin = (ops.PackedLinear.from_weight_mxfp4 if fp8 == 'fp4' else ops.PackedLinear.from_weight_fp8 if fp8 else ops.PackedLinear.from_weight)(w, b)
        for M in (1, 7, 8, 9, 16, 17, 32, 33, 64):
            x = rnd((M, K), 10 + M)
            res = rnd((M, N), 4)
            print('sha', N, K, fp8, M, sha(ops.gemm(x, lin, residual=res)))
            if M in (8, 32) and N % 16 == 0:
                for sk in (3, 4):
                    part = torch.zeros((sk, M, N), dtype=torch.float32, device='cuda')
                    ops.gemm_splitk(x, lin, part, sk)
                    print('sha split', N, K, fp8, M, sk, sha(part))
        T = 40
        rows = torch.tensor([3, 9, 11, 20, 21, 22, 30, 31, 38, 39], dtype=torch.int32, device='cuda')
        xs = rnd((T, K), 77)
        o = torch.zeros((T, N), dtype=BF16, device='cuda')
        ops.gemm(xs, lin, out=o, M=10, row_idx=rows)
        print('sha rows', N, K, fp8, sha(o))
g, u = rnd((1024, 3584), 6, 0.02), rnd((1024, 3584), 7, 0.02)
for fp8 in (False, True, 'fp4'):
    lin = (ops.PackedLinear.from_gate_up_mxfp4 if fp8 == 'fp4' else ops.PackedLinear.from_gate_up_fp8 if fp8 else ops.PackedLinear.from_gate_up)(g, u)
    for M in (8, 24, 48):
        print('sha swiglu', fp8, M, sha(ops.gemm(rnd((M, 3584), 8), lin)))
"""
    shas = {}
    for xl in ("0", "default"):
        env = dict(os.environ)
        if xl == "0":
            env.update(UMV_SKINNY_XL="0")
        r = sp.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        shas[xl] = [ln for ln in r.stdout.splitlines() if ln.startswith("sha")]
        assert len(shas[xl]) > 90, len(shas[xl])
    assert shas["0"] == shas["default"], [(a, b) for a, b in zip(shas["0"], shas["default"]) if a != b][:10]


def test_mid_batch_full_line_x_staging_bit_identical(ops):
    """33..64-row wide-N GEMMs (128 x 64 tile, UMV_GEMM_M64_TILED 2 = full-line x staging, k-steps of 32; 1 = k-steps of 64, half lines)
    and the 65..128-row split-K tile (UMV_SPLITK_TILED_XL 1 / 0): same operands, same k order per accumulator - every bit must agree.
    Ragged rows, K % 64 != 0, odd K-range starts (K = 3584 over 3 / 7 splits), SwiGLU, bias + residual, row-indexed x."""
    import subprocess as sp
    code = f"""
import hashlib, sys, math, torch
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
from unimedvl_amd import ops
from test_kernel_branches_gpu import rnd, BF16
def sha(t): return hashlib.sha256(t.cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32).numpy().tobytes()).hexdigest()[:16]
g, u = rnd((1024, 3584), 6, 0.02), rnd((1024, 3584), 7, 0.02)
glin = ops.PackedLinear.from_gate_up(g, u)
for M in (33, 40, 47, 64):
    print('sha swiglu', M, sha(ops.gemm(rnd((M, 3584), 8), glin)))
for N, K in ((16384, 3584), (18944, 1096), (20000, 4304)):
    w = rnd((N, K), 2, 1 / math.sqrt(K)); b = rnd((N,), 3)
    lin = ops.PackedLinear.from_weight(w, b)
    for M in (33, 50, 64):
        x = rnd((M, K), 10 + M); res = rnd((M, N), 4)
        print('sha wide', N, K, M, sha(ops.gemm(x, lin, residual=res)))
    T = 80
    rows = torch.randperm(T, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5))[:45].sort().values.to(torch.int32)
    xs = rnd((T, K), 77); o = torch.zeros((T, N), dtype=BF16, device='cuda')
    ops.gemm(xs, lin, out=o, M=45, row_idx=rows)
    print('sha rows', N, K, sha(o))
for N, K in ((3584, 3584), (4608, 3584), (3584, 18944), (1008, 1096)):
    w = rnd((N, K), 2, 1 / math.sqrt(K))
    lin = ops.PackedLinear.from_weight(w)
    for M in (65, 96, 127, 128):
        x = rnd((M, K), 10 + M)
        for sk in (2, 3, 7):
            part = torch.zeros((sk, M, N), dtype=torch.float32, device='cuda')
            ops.gemm_splitk(x, lin, part, sk)
            print('sha split', N, K, M, sk, sha(part))
"""
    shas = {}
    for v in ("old", "default"):
        env = dict(os.environ)
        if v == "old":
            env.update(UMV_GEMM_M64_TILED="1", UMV_SPLITK_TILED_XL="0")
        r = sp.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        shas[v] = [ln for ln in r.stdout.splitlines() if ln.startswith("sha")]
        assert len(shas[v]) == 4 + 3 * 4 + 4 * 12, len(shas[v])
    assert shas["old"] == shas["default"], [(a, b) for a, b in zip(shas["old"], shas["default"]) if a != b][:10]


# ---------------------------------------------------------------------------------------------------------- attention
def _attn_ref(q, ks, vs, q_lens, causal):
    """flash-attn model in fp32 on the device: S = QK^T/sqrt(d) (+ bottom-right causal mask), fp32 softmax, P rounded to
    bf16 before PV, fp32 accumulate, one division, bf16 out (oracle/unimedvl_cpu.py::attention_segment impl='flash')."""
    out = torch.empty_like(q)
    t0 = 0
    for i, lq in enumerate(q_lens):
        k, v = ks[i], vs[i]
        lk = k.shape[0]
        rep = q.shape[1] // k.shape[1]
        qf = q[t0:t0 + lq].float().transpose(0, 1)
        kf = k.float().transpose(0, 1).repeat_interleave(rep, dim=0)
        vf = v.float().transpose(0, 1).repeat_interleave(rep, dim=0)
        s = qf @ kf.transpose(1, 2) / math.sqrt(q.shape[-1])
        if causal:
            mask = torch.ones(lq, lk, dtype=torch.bool, device=q.device).tril(diagonal=lk - lq)
            s = s.masked_fill(~mask, float("-inf"))
        m = s.max(-1, keepdim=True).values
        p = torch.exp(s - m)
        l = p.sum(-1, keepdim=True)
        o = (p.to(BF16).float() @ vf) / l
        out[t0:t0 + lq] = o.transpose(0, 1).to(BF16)
        t0 += lq
    return out


def _attn_run(ops, nq, nkv, hd, q_lens, k_lens, causal, seed, want_tq):
    lib = _lib()
    nseg = len(q_lens)
    tq = lib.umv_attn_prefill_tq(nseg, nq, nkv, hd, max(q_lens))
    assert tq == want_tq, f"policy moved: this case now runs TQ={tq}, the test is meant to pin TQ={want_tq}"
    cap = (max(k_lens) + 31) // 32 * 32
    slab = ops.KVSlab(nseg, nkv, cap, hd, "cuda")
    slab.k.fill_(1e4)          # a key / value beyond kv_len that is not masked (p = 0 exactly) wrecks the output
    slab.vt.fill_(1e4)
    T = sum(q_lens)
    q = rnd((T, nq, hd), seed)
    ks = [rnd((lk, nkv, hd), seed + 1 + i) for i, lk in enumerate(k_lens)]
    vs = [rnd((lk, nkv, hd), seed + 100 + i) for i, lk in enumerate(k_lens)]
    for i, lk in enumerate(k_lens):
        slab.k[i, :, :lk] = ks[i].transpose(0, 1)
        slab.vt[i, :, :, :lk] = vs[i].permute(1, 2, 0)
    cu = torch.tensor([0] + list(torch.tensor(q_lens).cumsum(0)), dtype=torch.int32).cuda()
    out = torch.zeros((T, nq, hd), dtype=BF16, device="cuda")
    ops.attention(q, out, slab, cu, torch.tensor(k_lens, dtype=torch.int32).cuda(), nq, nkv, hd, causal, max(q_lens), max(k_lens))
    ref = _attn_ref(q, ks, vs, q_lens, causal)
    assert torch.isfinite(out.float()).all()
    err = (out.float() - ref.float()).abs().max().item()
    assert err < 0.03, f"attention max abs err {err}"
    # online softmax in key blocks vs one global max: P is rounded to bf16 against a different running max, so single
    # elements move by a few ulp; bound the tail and require the bulk to agree
    check_bf16(out, ref, 4, 0.5, f"attention hd{hd} TQ{want_tq}")
    return out


def test_attn_prefill_tq2_llm_image_span(ops):
    """8 x 1026-token image spans, non-causal, GQA 28/4, hd 128 (bagel.py:523-615 -> qwen2_navit.py:605-614): 1824 workgroups"""
    _attn_run(ops, 28, 4, 128, [1026] * 8, [1026] * 8, False, 50, want_tq=2)


def test_attn_prefill_tq2_causal_with_context(ops):
    """ragged causal prefill on top of cached context (text after an image): bottom-right aligned mask, 32-key stages"""
    _attn_run(ops, 28, 4, 128, [700, 513, 640, 1000], [700 + 1026, 513 + 40, 640, 1000 + 7], True, 60, want_tq=2)


def test_attn_prefill_tq2_flow_pass(ops):
    """12 segments of 258 query tokens over prompt + own tokens (a guided flow step of 4 images x 3 contexts, bagel.py:1120-1171)"""
    _attn_run(ops, 28, 4, 128, [258] * 12, [130 + 258] * 4 + [258] * 4 + [130 + 258] * 4, False, 70, want_tq=2)


def test_attn_prefill_tq2_vit_hd72(ops):
    """8 x 1024 patches, 16 heads of 72 (siglip_navit.py:232-241), and the ragged NaViT form"""
    _attn_run(ops, 16, 16, 72, [1024] * 8, [1024] * 8, False, 80, want_tq=2)
    _attn_run(ops, 16, 16, 72, [1024, 512, 768, 1024, 256, 1000], [1024, 512, 768, 1024, 256, 1000], False, 81, want_tq=2)


def test_attn_prefill_tq1_still_covered(ops):
    _attn_run(ops, 28, 4, 128, [1026], [1026], False, 90, want_tq=1)
    _attn_run(ops, 16, 16, 72, [1024], [1024], False, 91, want_tq=1)


@pytest.mark.parametrize("lens", [[1024] * 8, [1024, 512, 768, 1000, 256, 77], [1024], [77, 40], [5, 3]])
def test_attn_in_place_qk_equals_slab_form(ops, lens):
    """The cache-less self-attention form of the SigLIP tower (siglip_navit.py:222-241): q and K are read where the QKV GEMM wrote
    them - column slices of the fused [T, 3*1152] buffer (q_row_stride / k_key_stride) - and only V goes through qkv_post
    (V-only split into V^T).  Same bits as the slab form (q copy + K slab), on the LDS-shared kernels (TQ = 2, TQ = 1) and on
    the per-wave kernel (tiny segments), ragged lengths included."""
    nh, hd = 16, 72
    T, nseg = sum(lens), len(lens)
    qkv = rnd((T, 3 * nh * hd), 500 + T)
    cap = (max(lens) + 31) // 32 * 32
    seg = torch.cat([torch.full((n,), i, dtype=torch.int32) for i, n in enumerate(lens)]).cuda()
    slot = torch.cat([torch.arange(n, dtype=torch.int32) for n in lens]).cuda()
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32).cuda()
    kvl = torch.tensor(lens, dtype=torch.int32).cuda()
    # slab form
    slab = ops.KVSlab(nseg, nh, cap, hd, "cuda")
    q = torch.zeros((T, nh, hd), dtype=BF16, device="cuda")
    ops.qkv_post(qkv, q, slab, seg, slot, None, nh, nh, hd)
    ref = torch.zeros((T, nh * hd), dtype=BF16, device="cuda")
    ops.attention(q, ref, slab, cu, kvl, nh, nh, hd, False, max(lens), max(lens))
    # in-place form
    vslab = ops.KVSlab(nseg, nh, cap, hd, "cuda", keys=False)
    assert vslab.k is None
    ops.qkv_post(qkv, None, vslab, seg, slot, None, nh, nh, hd)
    assert torch.equal(vslab.vt, slab.vt)
    out = torch.zeros_like(ref)
    ops.attention(qkv[:, :nh * hd], out, vslab, cu, kvl, nh, nh, hd, False, max(lens), max(lens), k_packed=qkv[:, nh * hd:2 * nh * hd])
    assert torch.isfinite(out.float()).all() and out.float().abs().max() > 0
    assert torch.equal(out, ref)
    # and against the fp32 flash model
    ks = [qkv[int(cu[i]):int(cu[i + 1]), nh * hd:2 * nh * hd].reshape(-1, nh, hd) for i in range(nseg)]
    vs = [qkv[int(cu[i]):int(cu[i + 1]), 2 * nh * hd:].reshape(-1, nh, hd) for i in range(nseg)]
    model = _attn_ref(qkv[:, :nh * hd].reshape(T, nh, hd).contiguous(), ks, vs, lens, False)
    assert (out.view(T, nh, hd).float() - model.float()).abs().max().item() < 0.03


def test_attn_in_place_argument_errors(ops):
    from unimedvl_amd._lib import UmvError
    nh, hd, T = 16, 72, 64
    qkv = rnd((T, 3 * nh * hd), 7)
    cu = torch.tensor([0, T], dtype=torch.int32).cuda()
    kvl = torch.tensor([T], dtype=torch.int32).cuda()
    out = torch.zeros((T, nh * hd), dtype=BF16, device="cuda")
    vslab = ops.KVSlab(1, nh, 64, hd, "cuda", keys=False)
    with pytest.raises(UmvError):      # a keys=False slab without packed K
        ops.attention(qkv[:, :nh * hd], out, vslab, cu, kvl, nh, nh, hd, False, T, T)
    with pytest.raises(UmvError):      # packed K is the non-causal, unsplit form
        ops.attention(qkv[:, :nh * hd], out, vslab, cu, kvl, nh, nh, hd, True, T, T, k_packed=qkv[:, nh * hd:2 * nh * hd])
    with pytest.raises(UmvError):      # V-only split goes with a keys=False slab only
        ops.qkv_post(qkv, None, ops.KVSlab(1, nh, 64, hd, "cuda"), torch.zeros(T, dtype=torch.int32).cuda(),
                     torch.arange(T, dtype=torch.int32).cuda(), None, nh, nh, hd)


def _attn_ab(env):
    e = dict(os.environ, **env)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "attn_ab.py")], env=e, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if "sha" in ln]
    assert len(lines) >= 7, out.stdout
    return lines


def test_attn_kernel_variants_bit_identical():
    """tools/attn_ab.py as a test.  The exact-running-maximum family - the per-wave streaming kernel (UMV_ATTN_SHARED=0) and the LDS-shared
    kernels built with UMV_ATTN_LAZY=0, one q-tile per wave (UMV_ATTN_TQ=1) or two (UMV_ATTN_TQ=2) - produces the same bits on every shape
    of the script; so do the two shipped lazy-reference kernels (TQ = 1, TQ = 2) among themselves, under either packing of the q-tiles."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    sha = lambda lines: [ln.split("sha")[-1].split()[0] for ln in lines]
    wave = sha(_attn_ab({"UMV_ATTN_SHARED": "0"}))
    assert wave == sha(_attn_ab({"UMV_ATTN_TQ": "1", "UMV_ATTN_LAZY": "0"})) == sha(_attn_ab({"UMV_ATTN_TQ": "2", "UMV_ATTN_LAZY": "0"}))
    lazy1, lazy2 = sha(_attn_ab({"UMV_ATTN_TQ": "1"})), sha(_attn_ab({"UMV_ATTN_TQ": "2"}))
    assert lazy1 == lazy2, (lazy1, lazy2)
    assert lazy1 != wave          # (the lazy reference rounds P at another scale: same softmax, other bits)
    # the packing of the (token, head) pairs into q-tiles (dense: 16 per tile at G = 7; UMV_ATTN_DENSE=0: whole tokens, 14) changes no bit:
    # a row's keys, blocks and softmax reference are its own
    assert sha(_attn_ab({"UMV_ATTN_DENSE": "0"})) == lazy1
    assert sha(_attn_ab({"UMV_ATTN_DENSE": "0", "UMV_ATTN_LAZY": "0"})) == wave


def test_attn_lazy_softmax():
    """The shipped prefill attention (lazy softmax reference, csrc/attention_prefill.hip::attn_softmax_lazy) against EXACT fp32 attention,
    next to the exact-running-maximum kernels on the same inputs: measured mean |error| 9.2e-5 vs 8.7e-5, max 2-4e-3 either way (one bf16
    ulp of the output range); and the kernel is deterministic (the same call six times: a two-tiles-in-one-call form of the softmax was
    not - tools/attn_lazy_det.py)."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")

    def errs(lines):
        out = []
        for ln in lines:
            if "vs fp32" in ln:
                t = ln.split("vs fp32:")[1].split()
                out.append((float(t[1]), float(t[3])))
        return out

    exact, lazy = errs(_attn_ab({"UMV_ATTN_LAZY": "0", "ATTN_AB_REF": "1"})), errs(_attn_ab({"ATTN_AB_REF": "1"}))
    assert len(exact) == len(lazy) >= 6
    print("exact (max, mean):", exact)
    print("lazy  (max, mean):", lazy)
    for (mx0, mean0), (mx1, mean1) in zip(exact, lazy):
        assert mx1 <= max(2.0 * mx0, 4e-3) and mean1 <= 1.25 * mean0, (mx0, mean0, mx1, mean1)
    for env in ({"UMV_ATTN_TQ": "2"}, {"UMV_ATTN_TQ": "2", "SHAPE": "16,16,72,8", "L": "1024"}, {"UMV_ATTN_TQ": "1", "SHAPE": "28,4,128,2", "L": "1026"}):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "attn_lazy_det.py")], env=dict(os.environ, **env), capture_output=True,
                             text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        runs = [ln for ln in out.stdout.splitlines() if ln.startswith("run ")]
        assert len(runs) == 5 and all("tokens differing 0:" in ln for ln in runs), out.stdout


@pytest.mark.parametrize("M,N,K,epi", [(8208, 37888, 3584, "swiglu"), (8208, 3584, 18944, "residual"), (8192, 4304, 1152, "gelu"), (8192, 1152, 4304, "residual"),
                                      (2064, 4608, 3584, "bias"), (272, 4608, 3584, "bias"), (8, 37888, 3584, "swiglu"), (32, 3584, 18944, "residual")])
def test_gemm_race_screen(ops, M, N, K, epi):
    """Multi-run race screen of the hand-synchronised GEMM kernels at the shapes the bench legs run (counted vmcnt waits, LDS-DMA rings, one
    barrier per k-step: an early read "passes whenever the DMA happens to land first", guide section on LDS-DMA ordering; round 6 found a
    nondeterministic attention variant that every small-shape parity case had passed).  The same launch 25 times with all CUs busy: every
    output must equal the first bit for bit."""
    x = rnd((M, K), 11)
    if epi == "swiglu":
        I = N // 2
        lin = ops.PackedLinear.from_gate_up(rnd((I, K), 12, 1 / math.sqrt(K)), rnd((I, K), 13, 1 / math.sqrt(K)))
        kw, n_out = {}, I
    else:
        lin = ops.PackedLinear.from_weight(rnd((N, K), 12, 1 / math.sqrt(K)), rnd((N,), 14))
        kw, n_out = {}, N
        if epi == "residual":
            kw["residual"] = rnd((M, N), 15)
        elif epi == "gelu":
            kw["act"] = "gelu_tanh"
    first, bad = None, 0
    for _ in range(25):
        out = torch.zeros((M, n_out), dtype=BF16, device="cuda")
        ops.gemm(x, lin, out=out, **kw)
        if first is None:
            first = out
        else:
            bad += int(not torch.equal(out, first))
    assert torch.isfinite(first.float()).all() and bad == 0, f"{bad} of 24 repeats differ from the first launch"
