"""Interval reference of the six places that normalise a row with rsqrt_ieee(sum / n + eps) (csrc/norm.hip, csrc/qkv_post.hip, the
fused-RMSNorm prologue of csrc/gemm_skinny.h), on CPU tensors, and the seeded inputs the tests of those kernels share.

The kernels state their arithmetic as exact rounding chains (norm.hip: rmsnorm_kernel, residual_rmsnorm_kernel, layernorm_kernel;
qkv_post.hip: norm_rope_pair; gemm_skinny.h: the phase-2 normalisation).  The ONE thing a correct kernel may vary is the order of the
fp32 row sum, so the reference allows exactly that and nothing else:

  * the row statistic is taken in fp64 from the bf16 inputs (a bf16 square is exact in fp64): r64 = 1 / sqrt(ms64 + eps);
  * the kernel's fp32 rstd must lie in  [r_lo, r_hi] = r64 * (1 -+ DELTA)  rounded to fp32 outward, DELTA = 2^-17 relative;
  * every chain is evaluated in torch fp32 with explicit .to(bfloat16).float() roundings (the build uses -ffp-contract=off, so plain
    fp32 operations model the kernel) at BOTH ends; each single step is monotone in r, the two RoPE terms can move in opposite
    directions, so the interval is propagated term by term (min and max of each term, then the add, then the rounding);
  * the kernel's output must lie between the two bounds for every element, bf16 compared as ordered values (-0 below +0).  Where the
    bounds coincide the requirement is bit-exact.  No frac_exact, no ulp allowance, no absolute fallback.

DELTA.  The deepest summation in these kernels is rmsnorm_kernel<16>: 128 sequential adds per lane, 6 butterfly steps, and the
rowblock kernels add 2-3 cross-wave adds.  A sum of non-negative terms of depth d has a relative error <= d * 2^-24 (each add rounds
a partial sum that is no larger than the total); the squares, the division by H, the add of eps, the square root and the divide add
<= 5 * 2^-24.  rstd carries half of the relative error of its argument: (128 + 6 + 3 + 5) / 2 = 71, about 72 * 2^-24 < 2^-17 =
128 * 2^-24.  One value everywhere.

Chains (w, cos, sin: bf16 values; r: the fp32 rstd; rot = rotate_half):
    rms        bf16(w * bf16(x * r))                                           modeling_qwen2.py:89-94
    und RoPE   n = bf16(w * bf16(x * r));  bf16(bf16(n * cos) + bf16(rot(n) * sin))   qwen2_navit.py:544-545,576-583
    gen RoPE   n = w * (x * r) in fp32;    bf16(n * cos + rot(n) * sin)               qwen2_navit.py:568-583
    LayerNorm  bf16(((d * r) * w) + b),  d = x - mean                          F.layer_norm on bf16, fp32 statistics

LayerNorm inputs come from a grid on which every partial sum of the row is exact in fp32 in any order (x = m * 2^-k, integer
|m| <= 255, H <= 4096: |sum m| < 2^20), so mean = fp32(exact sum) / H is ONE fixed rounding, d = x - mean is fixed, and only the sum
of d^2 varies with the order: the same DELTA applies to its rstd.

Rows that leave the interval model have direct expectations (rms_bounds): a row whose fp32 sum of squares is +inf (one element 2^64)
has rstd = 0 exactly - zeros with the sign of w * x; a row holding a NaN is NaN everywhere."""
import math

import numpy as np
import torch

BF16 = torch.bfloat16
F64 = torch.float64
DELTA = 2.0 ** -17


def c32(c):
    """a constant as the fp32 value a kernel argument carries"""
    return float(np.float32(c))


def rb(t):
    """round an fp32 tensor through bf16 (the kernels' rbf)"""
    return t.to(BF16).float()


# ---------------------------------------------------------------------------------------------------------- ordered comparison
def key(t, signed_zero=True):
    """bf16 tensor -> int32 keys ordered like the values, -0 below +0 (signed_zero=False: both zeros on one key)"""
    i = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    mag = i & 0x7FFF
    k = torch.where(i >= 0x8000, -mag - 1, mag)
    if not signed_zero:
        k = torch.where(mag == 0, torch.zeros_like(k), k)
    return k


def order(a, b):
    """(min, max) of two bf16 tensors by key()"""
    sw = key(a) > key(b)
    return torch.where(sw, b, a), torch.where(sw, a, b)


def outside(got, lo, hi, signed_zero=True):
    """mask of the elements of got (bf16) that are NaN or not inside [lo, hi]"""
    assert got.shape == lo.shape == hi.shape and got.dtype == lo.dtype == hi.dtype == BF16, (got.shape, lo.shape, hi.shape)
    assert not bool(torch.isnan(lo.float()).any() | torch.isnan(hi.float()).any()), "a bound is NaN: the input family left the model"
    g = key(got, signed_zero)
    return torch.isnan(got.float()) | (g < key(lo, signed_zero)) | (g > key(hi, signed_zero))


def ambiguous(lo, hi, signed_zero=True):
    """share of elements whose two bounds differ"""
    return float((key(lo, signed_zero) != key(hi, signed_zero)).float().mean())


def report(got, lo, hi, signed_zero=True, nan_rows=None):
    """the figures a test asserts on: checked, outside, pinned (share of the elements whose bounds coincide: bit-exact requirement),
    first (index and values of the first element outside).  nan_rows: rows that must be NaN everywhere instead."""
    got, lo, hi = got.cpu(), lo.clone(), hi.clone()
    bad_nan = 0
    if nan_rows is not None and bool(nan_rows.any()):
        bad_nan = int((~torch.isnan(got[nan_rows].float())).sum())
        got = got.clone()
        got[nan_rows], lo[nan_rows], hi[nan_rows] = 0.0, 0.0, 0.0          # checked above: neutral for the interval part
    out = outside(got, lo, hi, signed_zero)
    first = None
    if bool(out.any()):
        idx = tuple(int(v) for v in out.nonzero()[0])
        first = dict(index=idx, got=float(got[idx]), lo=float(lo[idx]), hi=float(hi[idx]))
    return dict(checked=got.numel(), outside=int(out.sum()) + bad_nan, pinned=round(1.0 - ambiguous(lo, hi, signed_zero), 6), first=first)


# ---------------------------------------------------------------------------------------------------------- the row statistic
def _f32_outward(v64, up):
    f = v64.to(torch.float32)
    inf = torch.full_like(f, math.inf if up else -math.inf)
    wrong = (f.to(F64) < v64) if up else (f.to(F64) > v64)
    return torch.where(wrong, torch.nextafter(f, inf), f)


def rstd_interval(ms64, eps):
    """ms64: the fp64 row statistic [..., 1] -> (r_lo, r_hi) fp32: 1 / sqrt(ms + eps) * (1 -+ DELTA), rounded outward"""
    r64 = 1.0 / torch.sqrt(ms64 + c32(eps))
    assert bool(torch.isfinite(r64).all()), "eps = 0 on a row without energy: not a case of the model"
    return _f32_outward(r64 * (1.0 - DELTA), False), _f32_outward(r64 * (1.0 + DELTA), True)


def rms_stat(x):
    """fp64 mean of squares of the bf16 rows [..., H] -> [..., 1]"""
    return (x.to(F64) ** 2).sum(-1, keepdim=True) / x.shape[-1]


def rms_rstd(x, eps):
    """(r_lo, r_hi, nan_rows) of bf16 rows [..., H].  A row with an element whose square is +inf in fp32 has r_lo = r_hi = 0; every
    other row must stay below 2^127 in its sum of squares (no order of the fp32 sum overflows)."""
    x64 = x.to(F64)
    nan_rows = torch.isnan(x64).any(-1)
    x64 = torch.where(nan_rows[..., None], torch.zeros_like(x64), x64)
    over = ((x64 ** 2).amax(-1, keepdim=True) >= 2.0 ** 128)
    ss = (x64 ** 2).sum(-1, keepdim=True)
    assert bool((over | (ss < 2.0 ** 127)).all()), "a row's sum of squares may or may not overflow fp32: not a case of the model"
    ms = torch.where(over | nan_rows[..., None], torch.ones_like(ss), ss / x.shape[-1])      # (1: a placeholder, replaced below)
    lo, hi = rstd_interval(ms, eps)
    zero = torch.zeros_like(lo)
    return torch.where(over, zero, lo), torch.where(over, zero, hi), nan_rows


# ---------------------------------------------------------------------------------------------------------- the chains
def rms_chain(x, w, r):
    """bf16(w * bf16(x * r)); x [..., H] bf16, w broadcastable bf16, r [..., 1] fp32"""
    return (w.float() * rb(x.float() * r)).to(BF16)


def rms_bounds(x, w, eps, w_gen=None, expert=None):
    """(lo, hi, nan_rows) of the rms chain; expert (int [T], with w_gen): rows with a nonzero flag take w_gen"""
    ww = w[None, :] if w.dim() == 1 else w
    if expert is not None:
        ww = torch.where(expert.bool()[:, None], w_gen[None, :], w[None, :])
    r_lo, r_hi, nan_rows = rms_rstd(x, eps)
    xs = torch.where(nan_rows[..., None], torch.zeros_like(x), x)
    lo, hi = order(rms_chain(xs, ww, r_lo), rms_chain(xs, ww, r_hi))
    return lo, hi, nan_rows


def rot(n):
    h = n.shape[-1] // 2
    return torch.cat((-n[..., h:], n[..., :h]), dim=-1)


def rope_terms(x, w, cos, sin, r, gen):
    """the two terms of a chain at one rstd, fp32 tensors: (n * cos, rot(n) * sin), rounded through bf16 in the und chain"""
    if gen:
        n = w.float() * (x.float() * r)
        return n * cos.float(), rot(n) * sin.float()
    n = rb(w.float() * rb(x.float() * r))
    return rb(n * cos.float()), rb(rot(n) * sin.float())


def rope_bounds(x, w, cos, sin, eps, gen):
    """(lo, hi) of norm + RoPE.  x [T, heads, hd] bf16; w, cos, sin broadcastable to it (bf16)"""
    r_lo, r_hi, nan_rows = rms_rstd(x, eps)
    assert not bool(nan_rows.any())
    a1, a2 = rope_terms(x, w, cos, sin, r_lo, gen)
    b1, b2 = rope_terms(x, w, cos, sin, r_hi, gen)
    lo = (torch.minimum(a1, b1) + torch.minimum(a2, b2)).to(BF16)
    hi = (torch.maximum(a1, b1) + torch.maximum(a2, b2)).to(BF16)
    return lo, hi


def ln_parts(x):
    """(mean fp32 [T, 1], d fp32 [T, H], var64 [T, 1]) of grid rows: the exact sum rounded once, the fixed differences, the fp64
    mean of their squares"""
    H = x.shape[-1]
    s64 = x.to(F64).sum(-1, keepdim=True)
    assert bool((s64.to(torch.float32).to(F64) == s64).all()), "the row sum is not exact in fp32: not a grid row"
    mean = s64.to(torch.float32) / float(H)
    d = x.float() - mean
    return mean, d, (d.to(F64) ** 2).sum(-1, keepdim=True) / H


def ln_chain(d, w, b, r):
    return (((d * r) * w.float()) + b.float()).to(BF16)


def ln_bounds(x, w, b, eps):
    _, d, var = ln_parts(x)
    r_lo, r_hi = rstd_interval(var, eps)
    return order(ln_chain(d, w[None, :], b[None, :], r_lo), ln_chain(d, w[None, :], b[None, :], r_hi))


def seq_sum(p, bias=None):
    """the kernels' split sum: an fp32 accumulator that starts at +0 takes the splits in order 0..S-1, then the bias"""
    acc = torch.zeros_like(p[0])
    for s in range(p.shape[0]):
        acc = acc + p[s]
    return acc if bias is None else acc + bias.float()


# ---------------------------------------------------------------------------------------------------------- input families
RMS_SCALES = {"2^-40": -40, "2^-12": -12, "2^-10": -10, "2^0": 0, "2^20": 20, "2^50": 50}      # ms << eps at 2^-12, ms ~ eps at 2^-10
RMS_FINITE = tuple(RMS_SCALES) + ("zero", "onehot_last", "denormal")
RMS_ENERGY = tuple(RMS_SCALES) + ("onehot_last",)                        # the rows an eps = 0 launch may hold
RMS_SPECIAL = ("overflow", "nan")                                        # the rmsnorm entry point only: direct expectations
EPS_ALL = (1e-6, 1e-5, 1.0, 0.0)
EPS_TWO = (1e-6, 1.0)
EPS_LN = (1e-6, 1e-5, 1.0)


def _gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * m for s, m in zip(seed, (1, 1009, 1000003, 7919, 104729, 31))) % (2 ** 31))


def row_families(T, families, offset=0):
    return [families[(i + offset) % len(families)] for i in range(T)]


def rms_rows(T, H, families, offset=0, seed=0, dtype=BF16):
    """[T, H] rows, row i of family families[(i + offset) % len]: a seeded randn row scaled by 2^s, or a special row.  dtype=float32:
    the unrounded values (split-K partials)"""
    g = _gen(T, H, offset, seed)
    x = torch.randn(T, H, generator=g)
    m = torch.randint(-127, 128, (T, H), generator=g).float()
    for j in range(6):                           # |m| = 3 * 2^j steps aside: m * 1000 (rstd at eps = 1e-6) is an exact bf16 tie, which no interval can pin
        m = torch.where(m.abs() == 3 * 2 ** j, m + torch.sign(m), m)
    fam = row_families(T, families, offset)
    for i, f in enumerate(fam):
        if f in RMS_SCALES:
            x[i] *= 2.0 ** RMS_SCALES[f]
        elif f == "zero":
            x[i] = 0.0
        elif f == "onehot_last":                 # the only nonzero element sits in the last 16-byte chunk
            x[i] = 0.0
            x[i, H - 3] = 1.5
        elif f == "denormal":                    # bf16 denormals m * 2^-133: their squares are exactly 0 in fp32
            x[i] = m[i] * 2.0 ** -133
            x[i, 0] = 2.0 ** -133
        elif f == "overflow":                    # one square is +inf in fp32
            x[i, H // 2] = 2.0 ** 64
        elif f == "nan":
            x[i, H - 1] = math.nan
        else:
            raise ValueError(f)
    return x.to(dtype), fam


def rms_weight(H, seed):
    """1 + 0.1 randn with entries replaced by 0, -0, negative values and 2^+-8 (one of them in the last chunk)"""
    w = 1 + 0.1 * torch.randn(H, generator=_gen(H, seed, 77))
    w[1], w[2], w[3], w[4], w[5] = 0.0, -1.25, 256.0, 2.0 ** -8, -0.0
    w[H - 2] = -0.75
    if H > 16:
        w[H - 5] = 0.0
    return w.to(BF16)


def expert_flags(T, offset=0):
    return ((torch.arange(T) + offset) % 3 == 1).to(torch.int32)


LN_KINDS = tuple((k, kind) for k in (3, 10, 13) for kind in ("wide", "mean200", "narrow", "const"))


def ln_rows(T, H, offset=0, seed=0):
    """grid rows m * 2^-k: wide (|m| <= 255 around 0), mean200 (200 +- 8: a large mean, a small variance), narrow (+-2: at k = 13
    the variance is far below eps), const (out == b)"""
    assert H <= 4096
    g = _gen(T, H, offset, seed, 5)
    fam = row_families(T, LN_KINDS, offset)
    m = torch.empty(T, H)
    for i, (k, kind) in enumerate(fam):
        if kind == "wide":
            mi = torch.randint(-255, 256, (H,), generator=g)
        elif kind == "mean200":
            mi = 200 + torch.randint(-8, 9, (H,), generator=g)
        elif kind == "narrow":
            mi = torch.randint(-2, 3, (H,), generator=g)
        else:
            mi = torch.full((H,), 37 if i % 2 == 0 else -91)
        m[i] = mi.float() * 2.0 ** -k
    x = m.to(BF16)
    assert torch.equal(x.float(), m)
    return x, fam


def ln_weight_bias(H, seed):
    g = _gen(H, seed, 99)
    w = 1 + 0.1 * torch.randn(H, generator=g)
    b = 0.5 * torch.randn(H, generator=g)
    w[1], w[2], w[3], w[4] = 0.0, -1.25, 256.0, 2.0 ** -8
    w[H - 2] = -0.75
    b[2], b[3], b[H - 1] = 0.0, -3.0, 2.0 ** -8
    return w.to(BF16), b.to(BF16)


def rope_table(hd, rows=512, theta=1e6):
    """bf16 (cos, sin) [rows, hd].  Row 0 is position 0 (cos 1, sin 0); in every other row the second half carries a phase the first
    half does not, so that a kernel reading one half's entry for both elements of a rotate_half pair is wrong"""
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2).float() / hd))
    ang = torch.arange(rows).float()[:, None] * torch.cat((inv, inv))[None, :]
    ang[1:, hd // 2:] += 0.37
    return ang.cos().to(BF16), ang.sin().to(BF16)


# ---------------------------------------------------------------------------------------------------------- the cases of the GPU file
class Case(dict):
    __getattr__ = dict.__getitem__


RMS_SHAPES = (("rmsnorm_kernel<2>", 5, 8), ("rmsnorm_kernel<2>", 65, 1016), ("rmsnorm_kernel<2>", 65, 1024),
              ("rmsnorm_kernel<8>", 65, 1032), ("rmsnorm_kernel<8>", 65, 4096),
              ("rmsnorm_kernel<16>", 65, 4104), ("rmsnorm_kernel<16>", 65, 8192),
              ("rmsnorm_rowblock_kernel<2>", 1, 1024), ("rmsnorm_rowblock_kernel<2>", 64, 1024), ("rmsnorm_rowblock_kernel<2>", 3, 4096),
              ("rmsnorm_rowblock_kernel<4>", 5, 4104), ("rmsnorm_rowblock_kernel<4>", 64, 8192))


def _offsets(T, n):
    """launches of T rows that together hold all n families"""
    return range(0, n, T)


def rms_cases(shapes=RMS_SHAPES):
    """A: ops.rmsnorm.  Every eps without expert routing, EPS_TWO with w_gen / mixed expert; an eps = 0 launch holds no zero and no
    denormal row"""
    for kernel, T, H in shapes:
        w, w_gen = rms_weight(H, 1), rms_weight(H, 2)
        for routed in (False, True):
            for eps in (EPS_TWO if routed else EPS_ALL):
                fams = (RMS_ENERGY if eps == 0.0 else RMS_FINITE) + RMS_SPECIAL
                for off in _offsets(T, len(fams)):
                    x, fam = rms_rows(T, H, fams, off, seed=3)
                    yield Case(kernel=kernel, T=T, H=H, eps=eps, offset=off, x=x, fam=fam, w=w, w_gen=w_gen if routed else None,
                               expert=expert_flags(T, off) if routed else None)


RESIDUAL_SHAPES = tuple((H, S) for H in (256, 1024, 4096) for S in (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 64)) + \
                  tuple((H, S) for H in (4104, 8192) for S in (1, 2, 8))


def residual_inputs(S, T, H, offset, seed=0):
    """(partials fp32 [S, T, H], seq bf16 [T, H], families): partials and seq scaled together through the finite families"""
    p = torch.stack([rms_rows(T, H, RMS_FINITE, offset, seed=11 + 13 * s + seed, dtype=torch.float32)[0] for s in range(S)])
    seq, fam = rms_rows(T, H, RMS_FINITE, offset, seed=7 + seed)
    for i, f in enumerate(fam):
        if f == "onehot_last":                   # the one element arrives through the last split alone
            p[:, i] = 0.0
            p[S - 1, i, H - 3] = 1.5
            seq[i] = 0.0
    return p, seq, fam


def residual_cases(shapes=RESIDUAL_SHAPES):
    """B: ops.residual_rmsnorm, T = 1 (one launch, the families rotate with the case) and T = 5 (two launches: all nine families)"""
    for n, (H, S) in enumerate(shapes):
        w = rms_weight(H, 4)
        eps = EPS_LN[n % 3]
        for T, offs in ((1, (n % len(RMS_FINITE),)), (5, (0, 5))):
            for off in offs:
                p, seq, fam = residual_inputs(S, T, H, off)
                yield Case(H=H, S=S, T=T, eps=eps, offset=off, partials=p, seq=seq, fam=fam, w=w)


def residual_expect(c):
    """(new seq bf16, lo, hi) of a residual case"""
    new = (seq_sum(c.partials).to(BF16).float() + c.seq.float()).to(BF16)
    lo, hi, nan_rows = rms_bounds(new, c.w, c.eps)
    assert not bool(nan_rows.any())
    return new, lo, hi


GEMM_KS = (32, 256, 1024, 4096)
GEMM_MS = (1, 3, 8, 16)


def gemm_perm(K):
    return torch.randperm(K, generator=_gen(K, 123))


def gemm_cases():
    """C: the fused-RMSNorm prologue; x rows of the finite families, out[:, n] = the normalised x[:, perm[n]]"""
    for K in GEMM_KS:
        w = rms_weight(K, 5)
        for M in GEMM_MS:
            for e, eps in enumerate(EPS_TWO):
                off = (3 * M + 4 * e) % len(RMS_FINITE)
                x, fam = rms_rows(M, K, RMS_FINITE, off, seed=9)
                yield Case(K=K, M=M, eps=eps, offset=off, x=x, fam=fam, w=w)


NQ, NKV = 3, 1                                   # 5 heads: the item counts are no multiple of 4 or 16
NHEADS = NQ + 2 * NKV
QKV_TS = (1, 11, 64, 67)
QKV_HDS = (128, 72)
ROPE_ROWS = 512
SLAB_SEGS, SLAB_CAP, SLAB_FILL = 2, 64, 7.0


def qkv_layout(T):
    """(seg, slot, pos) int32 [T]: segment 0 takes its tokens from slot 8 on (aligned runs of 8), segment 1 from slot 3 on; the
    positions include 0, 1 and the last row of the table"""
    n0 = min(T, 40)
    seg = torch.cat((torch.zeros(n0), torch.ones(T - n0))).to(torch.int32)
    slot = torch.cat((torch.arange(8, 8 + n0), torch.arange(3, 3 + T - n0))).to(torch.int32)
    pos = ((torch.arange(T) * 37 + 5) % ROPE_ROWS).to(torch.int32)
    pos[0] = 0
    for i, v in ((1, 1), (2, ROPE_ROWS - 1)):
        if T > i:
            pos[i] = v
    if T == 1:
        pos[0] = ROPE_ROWS - 1
    return seg, slot, pos


def qkv_weights(hd):
    return tuple(rms_weight(hd, 20 + i) for i in range(4))         # q_norm, k_norm, q_norm_gen, k_norm_gen


def qkv_cases():
    """D: ops.qkv_post with norms from bf16 rows; each (token, head) row takes a finite family in turn"""
    for hd in QKV_HDS:
        for T in QKV_TS:
            for gen in (False, True):
                for e, eps in enumerate(EPS_TWO):
                    off = (T + 2 * e + gen) % len(RMS_FINITE)
                    rows, fam = rms_rows(T * NHEADS, hd, RMS_FINITE, off, seed=31)
                    yield Case(hd=hd, T=T, gen=gen, eps=eps, offset=off, x=rows.view(T, NHEADS, hd), fam=fam, partials=None, bias=None,
                               expert=expert_flags(T, 1) if gen else None)


QKV_PARTIAL_SS = (1, 4, 5, 8, 9)


def qkv_partial_cases():
    """D, from fp32 partials with a bias: x = bf16(sequential fp32 sum + bias), T = 8"""
    T = 8
    for hd in QKV_HDS:
        bias = (torch.randn(NHEADS * hd, generator=_gen(hd, 41)) * 2.0 ** -10).to(BF16)
        for n, S in enumerate(QKV_PARTIAL_SS):
            for gen in (False, True):
                eps = EPS_TWO[(n + gen) % 2]
                off = (n + 4 * gen) % len(RMS_FINITE)
                p = torch.stack([rms_rows(T * NHEADS, hd, RMS_FINITE, off, seed=51 + s, dtype=torch.float32)[0] for s in range(S)])
                fam = row_families(T * NHEADS, RMS_FINITE, off)
                for i, f in enumerate(fam):
                    if f == "onehot_last":
                        p[:S - 1, i] = 0.0
                p = p.view(S, T, NHEADS * hd)
                x = seq_sum(p, bias).to(BF16).view(T, NHEADS, hd)
                yield Case(hd=hd, T=T, gen=gen, eps=eps, offset=off, x=x, fam=fam, partials=p, bias=bias, S=S,
                           expert=expert_flags(T, 1) if gen else None)


def qkv_expect(c):
    """(q_lo, q_hi [T, NQ, hd], k_lo, k_hi [segs, NKV, cap, hd], vt [segs, NKV, hd, cap], layout): slab entries that no token
    addresses hold SLAB_FILL in both bounds"""
    hd, T = c.hd, c.T
    seg, slot, pos = qkv_layout(T)
    cos, sin = rope_table(hd, ROPE_ROWS)
    qn, kn, qg, kg = qkv_weights(hd)
    e = torch.zeros(T, dtype=torch.bool) if c.expert is None else c.expert.bool()
    wq = torch.where(e[:, None, None], qg[None, None, :], qn[None, None, :])
    wk = torch.where(e[:, None, None], kg[None, None, :], kn[None, None, :])
    cs, sn = cos[pos.long()][:, None, :], sin[pos.long()][:, None, :]
    q_lo, q_hi = rope_bounds(c.x[:, :NQ], wq, cs, sn, c.eps, c.gen)
    kl, kh = rope_bounds(c.x[:, NQ:NQ + NKV], wk, cs, sn, c.eps, c.gen)
    k_lo = torch.full((SLAB_SEGS, NKV, SLAB_CAP, hd), SLAB_FILL, dtype=BF16)
    k_hi = k_lo.clone()
    vt = torch.full((SLAB_SEGS, NKV, hd, SLAB_CAP), SLAB_FILL, dtype=BF16)
    for t in range(T):
        k_lo[seg[t], :, slot[t]] = kl[t]
        k_hi[seg[t], :, slot[t]] = kh[t]
        vt[seg[t], :, :, slot[t]] = c.x[t, NQ + NKV:]
    return q_lo, q_hi, k_lo, k_hi, vt, (seg, slot, pos)


LN_SHAPES = (("layernorm_kernel<3>", 1, 8), ("layernorm_kernel<3>", 5, 1528), ("layernorm_kernel<3>", 9, 1536),
             ("layernorm_kernel<8>", 5, 1544), ("layernorm_kernel<8>", 9, 4096))


def ln_cases(shapes=LN_SHAPES):
    """E: ops.layernorm"""
    for kernel, T, H in shapes:
        w, b = ln_weight_bias(H, 6)
        for eps in EPS_LN:
            for off in _offsets(T, len(LN_KINDS)):
                x, fam = ln_rows(T, H, off, seed=17)
                yield Case(kernel=kernel, T=T, H=H, eps=eps, offset=off, x=x, fam=fam, w=w, b=b)
