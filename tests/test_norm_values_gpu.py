"""The six places that normalise a row with rsqrt_ieee(sum / n + eps) - rmsnorm_kernel<2|8|16>, the rowblock tail shared by
rmsnorm_rowblock_kernel<2|4> and residual_rmsnorm_kernel<2|4, NS>, layernorm_kernel<3|8>, qkv_post_kernel<128|72>,
qk_post_vec128_kernel and the fused-RMSNorm prologue of the skinny GEMM - against the interval reference of tests/norm_ref.py (held to
the oracle, to a cap on its own width and to eleven wrong kernels by tests/test_norm_ref_cpu.py, on the same tensors).

Every output element must lie between the two bounds the reference derives from the ONE freedom a correct kernel has, the order of
its fp32 row sum; where the bounds coincide (>= 98.5 % of the elements) that is a bit-exact requirement.  No frac_exact, no ulp
allowance.  The inputs walk the magnitudes (rows 2^-40 .. 2^50 away from 1, ms << eps, ms ~ eps, all-zero, one element in the last
16-byte chunk, bf16 denormals, an overflowing sum, a NaN), eps in {1e-6, 1e-5, 1.0, 0} and every dispatch branch: the template
boundaries, the T <= 64 && H >= 1024 switch, expert routing, every NS of the split-K consumer, both RoPE chains, the fp32-partials
form.  Each check prints a line "REC {...}" (profiles/norm_values.txt is made of them; with UMV_NORM_VALUES_LOG=<file> the lines are
appended to that file too)."""
import json
import os

import pytest
import torch

import norm_ref as R

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd import ops as o
    return o


def umv_error():
    from unimedvl_amd import _lib
    return _lib.UmvError


def rec(kind, case, **kw):
    line = json.dumps(dict(where="gpu", kind=kind, case=case, **kw))
    print("REC " + line, flush=True)
    log = os.environ.get("UMV_NORM_VALUES_LOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")


class Tally:
    """the launches of one test: every launch is checked and counted, one record and one verdict at the end"""

    def __init__(self, kind, case):
        self.kind, self.case, self.checked, self.pinned, self.outside, self.launches, self.errors = kind, case, 0, 0.0, 0, 0, []

    def check(self, what, got, lo, hi, signed_zero=True, nan_rows=None):
        r = R.report(got, lo, hi, signed_zero, nan_rows)
        self.checked += r["checked"]
        self.pinned += r["pinned"] * r["checked"]
        self.outside += r["outside"]
        self.launches += 1
        if r["outside"]:
            self.errors.append(f"{self.kind} {self.case} {what}: {r['outside']} of {r['checked']} elements outside their bounds, first {r['first']}")

    def equal(self, what, got, want):
        nd = int((R.key(got.cpu()) != R.key(want)).sum())
        if nd:
            self.errors.append(f"{self.kind} {self.case} {what}: {nd} of {want.numel()} elements differ")

    def done(self):
        rec(self.kind, self.case, launches=self.launches, checked=self.checked, outside=self.outside,
            pinned_share=round(self.pinned / max(self.checked, 1), 6))
        assert self.launches > 0 and not self.errors, "\n".join(self.errors[:8])


# ---------------------------------------------------------------------------------------------------------- A. ops.rmsnorm
@pytest.mark.parametrize("kernel,T,H", R.RMS_SHAPES)
def test_rmsnorm(ops, kernel, T, H):
    """every family, eps in {1e-6, 1e-5, 1.0, 0} (an eps = 0 launch holds no zero and no denormal row), with and without w_gen / mixed
    expert.  The overflow row (one element 2^64: the fp32 sum is +inf, rstd 0) must be zeros with the sign of w * x, the NaN row NaN
    everywhere: both come out of rms_bounds as direct expectations."""
    t = Tally("A " + kernel, f"T={T} H={H}")
    for c in R.rms_cases([(kernel, T, H)]):
        lo, hi, nan_rows = R.rms_bounds(c.x, c.w, c.eps, c.w_gen, c.expert)
        got = ops.rmsnorm(c.x.cuda(), c.w.cuda(), c.eps, w_gen=None if c.w_gen is None else c.w_gen.cuda(),
                          expert=None if c.expert is None else c.expert.cuda())
        t.check(f"eps={c.eps} off={c.offset} routed={c.expert is not None}", got, lo, hi, nan_rows=nan_rows)
    t.done()


def test_rmsnorm_rejections(ops):
    w = R.rms_weight(8200, 1).cuda()
    for H in (8200, 12):
        with pytest.raises(umv_error()):
            ops.rmsnorm(torch.zeros((2, H), dtype=BF16, device="cuda"), w[:H].contiguous(), 1e-6)
    with pytest.raises(umv_error()):
        ops.rmsnorm(torch.zeros((2, 1024), dtype=BF16, device="cuda"), w[:1024].contiguous(), 1e-6,
                    expert=torch.zeros(2, dtype=torch.int32, device="cuda"))


# ---------------------------------------------------------------------------------------------------------- B. ops.residual_rmsnorm
@pytest.mark.parametrize("H", sorted({h for h, _ in R.RESIDUAL_SHAPES}))
def test_residual_rmsnorm(ops, H):
    """every split count of the dispatch (NS = 2, 3, 4, 6, 8 and the run-time loop at 1, 5, 7, 9, 16, 64; <4, 0> beyond H = 4096): the
    new seq is bit-equal to bf16(bf16(fp32 sum of the splits in order) + seq), out lies inside the rms interval of THAT seq"""
    t = Tally("B residual_rmsnorm_kernel", f"H={H}")
    for c in R.residual_cases([s for s in R.RESIDUAL_SHAPES if s[0] == H]):
        new, lo, hi = R.residual_expect(c)
        seq = c.seq.cuda()
        out = torch.full_like(seq, 7.0)
        ops.residual_rmsnorm(c.partials.cuda(), seq, c.w.cuda(), c.eps, out)
        t.equal(f"S={c.S} T={c.T} off={c.offset} new seq", seq, new)
        t.check(f"S={c.S} T={c.T} eps={c.eps} off={c.offset}", out, lo, hi)
    t.done()


# ---------------------------------------------------------------------------------------------------------- C. fused-RMSNorm GEMM prologue
@pytest.mark.parametrize("K", R.GEMM_KS)
def test_gemm_fused_rmsnorm_prologue(ops, K):
    """ops.gemm(x, lin, norm_w=, norm_eps=) with a permutation matrix as the weight (W[n, perm[n]] = 1, no bias): out[:, n] is the
    normalised x[:, perm[n]] bit for bit (the fp32 sum adds only zeros), which also pins the K indexing of the x staging.  Zeros are
    compared WITHOUT their sign: the accumulator starts at +0, so a normalised -0 arrives as +0."""
    perm = R.gemm_perm(K)
    W = torch.zeros((K, K), dtype=BF16)
    W[torch.arange(K), perm] = 1.0
    lin = ops.PackedLinear.from_weight(W.cuda())
    t = Tally("C gemm prologue", f"N=K={K}")
    for c in R.gemm_cases():
        if c.K != K:
            continue
        lo, hi, _ = R.rms_bounds(c.x, c.w, c.eps)
        got = ops.gemm(c.x.cuda(), lin, norm_w=c.w.cuda(), norm_eps=c.eps)
        t.check(f"M={c.M} eps={c.eps} off={c.offset}", got, lo[:, perm].contiguous(), hi[:, perm].contiguous(), signed_zero=False)
    t.done()


# ---------------------------------------------------------------------------------------------------------- D. ops.qkv_post with norms
def run_qkv(ops, t, c):
    q_lo, q_hi, k_lo, k_hi, vt, (seg, slot, pos) = R.qkv_expect(c)
    hd, T = c.hd, c.T
    slab = ops.KVSlab(R.SLAB_SEGS, R.NKV, R.SLAB_CAP, hd, "cuda")
    slab.k.fill_(R.SLAB_FILL)
    slab.vt.fill_(R.SLAB_FILL)
    q_out = torch.full((T, R.NQ, hd), R.SLAB_FILL, dtype=BF16, device="cuda")
    qn, kn, qg, kg = (w.cuda() for w in R.qkv_weights(hd))
    cos, sin = (v.cuda() for v in R.rope_table(hd, R.ROPE_ROWS))
    expert = None if c.expert is None else c.expert.cuda()
    qkv = None if c.partials is not None else c.x.reshape(T, R.NHEADS * hd).cuda()
    ops.qkv_post(qkv, q_out, slab, seg.cuda(), slot.cuda(), pos.cuda(), R.NQ, R.NKV, hd, c.eps, qn, kn,
                 qg if c.gen else None, kg if c.gen else None, expert, cos, sin, fp32_chain=c.gen,
                 partials=None if c.partials is None else c.partials.cuda(), bias=None if c.bias is None else c.bias.cuda())
    what = f"T={T} eps={c.eps} off={c.offset}" + (f" S={c.S}" if c.partials is not None else "")
    t.check(what + " q", q_out, q_lo, q_hi)
    k, sg, sl = slab.k.cpu(), seg.long(), slot.long()
    t.check(what + " K rows", k[sg, :, sl], k_lo[sg, :, sl], k_hi[sg, :, sl])
    k[sg, :, sl] = R.SLAB_FILL
    t.equal(what + " K slab entries no token addresses", k, torch.full_like(k, R.SLAB_FILL))
    t.equal(what + " V^T slab", slab.vt, vt)


@pytest.mark.parametrize("gen", [False, True])
@pytest.mark.parametrize("hd", R.QKV_HDS)
def test_qkv_post_norm_rope(ops, hd, gen):
    """nq = 3, nkv = 1 (5 heads: the `live` / `item >=` guards), T in {1, 11, 64, 67}: hd 128 at T >= 64 takes qk_post_vec128_kernel +
    v_transpose_kernel, everything else the per-head wave.  und chain, and the gen chain with mixed expert rows.  q rows and K slab
    rows inside the RoPE interval, V^T columns exact copies, untouched slab entries keep their fill."""
    t = Tally(f"D {'gen' if gen else 'und'} RoPE", f"hd={hd}")
    for c in R.qkv_cases():
        if c.hd == hd and c.gen == gen:
            run_qkv(ops, t, c)
    t.done()


@pytest.mark.parametrize("hd", R.QKV_HDS)
def test_qkv_post_norm_rope_from_partials(ops, hd):
    """the same from fp32 split-K partials with a bias, S in {1, 4, 5, 8, 9} (the four-wide, eight-wide and run-time split sums), both
    chains: x = bf16(sequential fp32 sum + bias)"""
    t = Tally("D RoPE from partials", f"hd={hd}")
    for c in R.qkv_partial_cases():
        if c.hd == hd:
            run_qkv(ops, t, c)
    t.done()


def test_qkv_post_rejects_other_head_dims(ops):
    hd, T = 64, 2
    slab = ops.KVSlab(1, R.NKV, 32, hd, "cuda")
    z = lambda *s: torch.zeros(s, dtype=BF16, device="cuda")
    i = torch.zeros(T, dtype=torch.int32, device="cuda")
    with pytest.raises(umv_error()):
        ops.qkv_post(z(T, R.NHEADS * hd), z(T, R.NQ, hd), slab, i, i, i, R.NQ, R.NKV, hd, 1e-6, z(hd), z(hd), cos_tab=z(4, hd), sin_tab=z(4, hd))


# ---------------------------------------------------------------------------------------------------------- E. ops.layernorm
@pytest.mark.parametrize("kernel,T,H", R.LN_SHAPES)
def test_layernorm(ops, kernel, T, H):
    """grid rows (every partial sum exact in fp32: the mean is one fixed rounding): wide, large mean with a small variance, variance
    far below eps, constant rows (out == b)"""
    t = Tally("E " + kernel, f"T={T} H={H}")
    for c in R.ln_cases([(kernel, T, H)]):
        lo, hi = R.ln_bounds(c.x, c.w, c.b, c.eps)
        got = ops.layernorm(c.x.cuda(), c.w.cuda(), c.b.cuda(), c.eps)
        t.check(f"eps={c.eps} off={c.offset}", got, lo, hi)
    t.done()


def test_layernorm_rejections(ops):
    w = torch.ones(4104, dtype=BF16, device="cuda")
    for H in (4104, 12):
        with pytest.raises(umv_error()):
            ops.layernorm(torch.zeros((2, H), dtype=BF16, device="cuda"), w[:H].contiguous(), w[:H].contiguous(), 1e-6)
