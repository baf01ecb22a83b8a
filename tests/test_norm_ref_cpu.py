"""The interval reference of the norm kernels (tests/norm_ref.py) itself, on the CPU: it contains the oracle's restatement of the model
code on every input family, its intervals are narrow enough to pin (the ambiguity cap is a CONDITION on the families, not a
measurement), and it rejects eleven wrong kernels.  tests/test_norm_values_gpu.py compares the kernels with this reference on the very
same tensors (both files take them from norm_ref).  Each check prints a line "REC {...}" (profiles/norm_values.txt is made of them;
with UMV_NORM_VALUES_LOG=<file> the lines are appended to that file too)."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import norm_ref as R
from oracle.unimedvl_cpu import apply_rope, rmsnorm

BF16, F64 = R.BF16, R.F64
CAP_RMS, CAP_LN = 0.01, 0.015                    # the share of elements whose two bounds may differ, per case of the GPU file and per input family


def rec(kind, case, **kw):
    line = json.dumps(dict(where="cpu", kind=kind, case=case, **kw))
    print("REC " + line, flush=True)
    log = os.environ.get("UMV_NORM_VALUES_LOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")


def rows_of(fam, *names):
    return torch.tensor([f in names for f in fam])


_cache = {}


def cached(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def rms_all():
    return cached("rms", lambda: [(c,) + R.rms_bounds(c.x, c.w, c.eps, c.w_gen, c.expert) for c in R.rms_cases()])


def residual_all():
    return cached("res", lambda: [(c,) + R.residual_expect(c) for c in R.residual_cases()])


def gemm_all():
    return cached("gemm", lambda: [(c,) + R.rms_bounds(c.x, c.w, c.eps)[:2] for c in R.gemm_cases()])


def qkv_all():
    return cached("qkv", lambda: [(c,) + R.qkv_expect(c) for c in list(R.qkv_cases()) + list(R.qkv_partial_cases())])


def ln_all():
    return cached("ln", lambda: [(c,) + R.ln_bounds(c.x, c.w, c.b, c.eps) for c in R.ln_cases()])


# ---------------------------------------------------------------------------------------------------------- the pieces
def test_outward_rounding_and_order():
    v = torch.tensor([1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, 1.0, 3.0e-40, 1.0e30], dtype=F64)
    lo, hi = R._f32_outward(v, False), R._f32_outward(v, True)
    assert bool((lo.to(F64) <= v).all() and (hi.to(F64) >= v).all())
    assert bool((torch.nextafter(lo, torch.full_like(lo, float("inf"))).to(F64) > v)[:2].all())
    assert bool((lo == hi)[2]) and not bool((lo == hi)[:2].any())
    r_lo, r_hi = R.rstd_interval(torch.tensor([[0.0], [1.0], [2.0 ** -80]], dtype=F64), 1e-6)
    r = 1.0 / torch.sqrt(torch.tensor([[0.0], [1.0], [2.0 ** -80]], dtype=F64) + R.c32(1e-6))
    assert bool((r_lo.to(F64) < r).all() and (r_hi.to(F64) > r).all())
    assert bool(((r_hi.to(F64) - r_lo.to(F64)) / r < 2.0 ** -15.9).all())
    t = torch.tensor([-float("inf"), -2.0, -2.0 ** -133, -0.0, 0.0, 2.0 ** -133, 1.0, float("inf")]).to(BF16)
    k = R.key(t)
    assert bool((k[1:] > k[:-1]).all()), "keys must be strictly ordered, -0 below +0"
    k0 = R.key(t, signed_zero=False)
    assert int(k0[3]) == int(k0[4]) and bool((k0[1:] >= k0[:-1]).all())
    assert bool(R.outside(torch.tensor([float("nan")]).to(BF16), t[:1], t[-1:]).all())
    assert bool(R.outside(t[3:4], t[4:5], t[4:5]).all()) and not bool(R.outside(t[3:4], t[4:5], t[4:5], signed_zero=False).any())


def test_families_are_what_they_claim():
    x, fam = R.rms_rows(11, 1024, R.RMS_FINITE + R.RMS_SPECIAL, 0, seed=3)
    assert fam == list(R.RMS_FINITE + R.RMS_SPECIAL)
    ms = R.rms_stat(torch.nan_to_num(x.float(), nan=0.0).to(BF16))[:, 0]
    assert 2.0 ** -25 < ms[1] < 2.0 ** -23 and 2.0 ** -21 < ms[2] < 2.0 ** -19          # ms << eps, ms ~ eps (1e-6 = 2^-19.9)
    assert float(x[5].float().pow(2).sum()) * 8 < 2.0 ** 127                           # 2^50 rows: H x^2 below 2^127 at H = 8192
    assert not bool(x[6].float().any())
    assert int((x[7] != 0).sum()) == 1 and bool(x[7, -8:].float().any())
    d = x[8].float()
    assert bool((d.abs() < 2.0 ** -126).all()) and int((d != 0).sum()) > 1000, "bf16 denormals, kept by the conversion"
    assert bool((d * d == 0).all()), "their squares are exactly 0 in fp32"
    assert float((x[9].float() ** 2).max()) == float("inf") and bool(torch.isnan(x[10].float()).any())
    w = R.rms_weight(8, 1).float()
    assert int((w == 0).sum()) >= 2 and bool((w < 0).any()) and bool((w == 256).any()) and bool((w == 2.0 ** -8).any())
    cos, sin = R.rope_table(128)
    assert bool((cos[0] == 1).all() and (sin[0] == 0).all()) and not torch.equal(cos[1:, :64], cos[1:, 64:])
    for c, lo, hi in ln_all():
        assert c.H <= 4096 and bool((c.x.float().abs() * 2.0 ** 13 <= 255 * 2.0 ** 10).all())


def test_special_rows_have_direct_expectations():
    """the overflow row: rstd = 0, zeros with the sign of w * x; the NaN row: flagged, not bounded"""
    x, fam = R.rms_rows(2, 1024, R.RMS_SPECIAL, 0, seed=3)
    w = R.rms_weight(1024, 1)
    lo, hi, nan_rows = R.rms_bounds(x, w, 1e-6)
    assert nan_rows.tolist() == [False, True]
    assert torch.equal(R.key(lo[0]), R.key(hi[0])) and not bool(lo[0].float().any())
    neg = torch.signbit(w.float()) ^ torch.signbit(x[0].float())
    assert torch.equal(torch.signbit(lo[0].float()), neg)
    good = lo.clone()
    good[1] = float("nan")
    assert R.report(good, lo, hi, nan_rows=nan_rows)["outside"] == 0
    good[1, 5] = 0.0
    assert R.report(good, lo, hi, nan_rows=nan_rows)["outside"] == 1


# ---------------------------------------------------------------------------------------------------------- 1. the oracle lies inside
def test_oracle_rmsnorm_inside():
    n = 0
    for c, lo, hi, nan_rows in rms_all():
        if c.eps == 0.0:
            continue
        keep = ~rows_of(c.fam, *R.RMS_SPECIAL)
        x = c.x[keep]
        ref = rmsnorm(x, c.w, c.eps)
        if c.expert is not None:
            e = c.expert.bool()[keep]
            ref[e] = rmsnorm(x[e], c.w_gen, c.eps)
        out = R.outside(ref, lo[keep], hi[keep])
        assert not bool(out.any()), f"oracle rmsnorm outside the interval: {c.kernel} T={c.T} H={c.H} eps={c.eps}: {int(out.sum())}"
        n += ref.numel()
    for c, new, lo, hi in residual_all():
        assert not bool(R.outside(rmsnorm(new, c.w, c.eps), lo, hi).any()), f"residual H={c.H} S={c.S} T={c.T}"
    for c, lo, hi in gemm_all():
        assert not bool(R.outside(rmsnorm(c.x, c.w, c.eps), lo, hi).any()), f"gemm K={c.K} M={c.M}"
    rec("oracle", "rmsnorm", elements=n, outside=0)


def oracle_rope(c):
    """apply_rope over rmsnorm as tests/test_kernels_gpu.py states the two chains"""
    seg, slot, pos = R.qkv_layout(c.T)
    cos, sin = R.rope_table(c.hd, R.ROPE_ROWS)
    qn, kn, qg, kg = R.qkv_weights(c.hd)
    q, k = c.x[:, :R.NQ], c.x[:, R.NQ:R.NQ + R.NKV]
    cs, sn = cos[pos.long()], sin[pos.long()]
    if not c.gen:
        return apply_rope(rmsnorm(q, qn, c.eps), rmsnorm(k, kn, c.eps), cs, sn)
    e = c.expert.bool()
    qf, kf = q.float(), k.float()
    qf[~e] = rmsnorm(qf[~e], qn, c.eps); qf[e] = rmsnorm(qf[e], qg, c.eps)
    kf[~e] = rmsnorm(kf[~e], kn, c.eps); kf[e] = rmsnorm(kf[e], kg, c.eps)
    qr, kr = apply_rope(qf, kf, cs, sn)
    return qr.to(BF16), kr.to(BF16)


def test_oracle_rope_inside():
    n = 0
    for c, q_lo, q_hi, k_lo, k_hi, vt, (seg, slot, pos) in qkv_all():
        qr, kr = oracle_rope(c)
        what = f"hd={c.hd} T={c.T} gen={c.gen} eps={c.eps} partials={c.partials is not None}"
        assert not bool(R.outside(qr, q_lo, q_hi).any()), "oracle q outside: " + what
        for t in range(c.T):
            assert not bool(R.outside(kr[t], k_lo[seg[t], :, slot[t]], k_hi[seg[t], :, slot[t]]).any()), "oracle k outside: " + what
        n += qr.numel() + kr.numel()
    rec("oracle", "rope", elements=n, outside=0)


def test_torch_layer_norm_mostly_inside():
    """F.layer_norm on bf16 uses another algorithm: >= 99 % of its elements inside, over all elements of the LayerNorm cases.  What it
    misses is its own error: its mean of a constant row is not the constant (so d != 0, times rstd = 1000 at eps = 1e-6: up to 18 % of
    such a row moves by one bf16 value), and a few elements of the large-mean rows.  The reference's constant rows ARE b, bit for bit."""
    per_shape, tot = {}, [0, 0]
    for c, lo, hi in ln_all():
        ref = F.layer_norm(c.x, (c.H,), c.w, c.b, c.eps)
        s = per_shape.setdefault((c.T, c.H), [0, 0])
        n_out_ = int(R.outside(ref, lo, hi).sum())
        s[0], s[1], tot[0], tot[1] = s[0] + n_out_, s[1] + ref.numel(), tot[0] + n_out_, tot[1] + ref.numel()
        const = torch.tensor([k[1] == "const" for k in c.fam])
        nz = c.b.float() != 0
        want = R.key(c.b[nz].expand(int(const.sum()), -1))
        assert torch.equal(R.key(lo[const][:, nz]), want) and torch.equal(R.key(hi[const][:, nz]), want), "constant rows: out == b"
    for (T, H), (o, n) in per_shape.items():
        rec("oracle", f"F.layer_norm T={T} H={H}", elements=n, share_inside=round(1.0 - o / n, 5))
    share = 1.0 - tot[0] / tot[1]
    rec("oracle", "F.layer_norm", elements=tot[1], share_inside=round(share, 5))
    assert share >= 0.99, f"only {share:.4f} of F.layer_norm inside the interval"


# ---------------------------------------------------------------------------------------------------------- 2. the ambiguity cap
def test_ambiguity_cap():
    """A condition on the inputs: per case of the GPU file - all launches of one shape and eps, which together hold every family (a
    single row is lumpy: its elements share one rstd, so one unlucky mantissa is 1 / 128 of the row) - at most 1 % (LayerNorm 1.5 %)
    of the elements have two different bounds."""
    groups = {}

    def add(kind, case, lo, hi, cap, signed_zero=True):
        g = groups.setdefault((kind, case), [0, 0, cap])
        g[0] += int((R.key(lo, signed_zero) != R.key(hi, signed_zero)).sum())
        g[1] += lo.numel()

    fams = {}

    def by_family(chain, fam, lo, hi):
        """rows [n, H] with their families: pooled over every launch of the chain, held to the same cap"""
        d = (R.key(lo) != R.key(hi)).sum(-1)
        for f, n in zip(fam, d.tolist()):
            g = fams.setdefault((chain, str(f)), [0, 0])
            g[0], g[1] = g[0] + n, g[1] + lo.shape[-1]

    for c, lo, hi, _ in rms_all():
        add(f"A {c.kernel}", f"T={c.T} H={c.H} eps={c.eps} routed={c.expert is not None}", lo, hi, CAP_RMS)
        by_family("rms", c.fam, lo, hi)
    for c, new, lo, hi in residual_all():
        add("B residual_rmsnorm_kernel", f"H={c.H} S={c.S}", lo, hi, CAP_RMS)
    for c, lo, hi in gemm_all():
        add("C gemm prologue", f"K={c.K} eps={c.eps}", lo, hi, CAP_RMS, signed_zero=False)
    for c, q_lo, q_hi, k_lo, k_hi, vt, (seg, slot, pos) in qkv_all():
        kind = f"D {'gen' if c.gen else 'und'} RoPE" + (" from partials" if c.partials is not None else "")
        k_rows = lambda k: torch.stack([k[seg[t], :, slot[t]] for t in range(c.T)])
        add(kind, f"hd={c.hd} eps={c.eps}", torch.cat((q_lo, k_rows(k_lo)), 1), torch.cat((q_hi, k_rows(k_hi)), 1), CAP_RMS)
        q_fam = [c.fam[t * R.NHEADS + h] for t in range(c.T) for h in range(R.NQ)]
        by_family("gen RoPE" if c.gen else "und RoPE", q_fam, q_lo.reshape(-1, c.hd), q_hi.reshape(-1, c.hd))
    for c, lo, hi in ln_all():
        add(f"E {c.kernel}", f"T={c.T} H={c.H} eps={c.eps}", lo, hi, CAP_LN)
        by_family("LayerNorm", [f"k={k} {kind}" for k, kind in c.fam], lo, hi)
    for (chain, f), (a, n) in fams.items():
        rec("ambiguity by family", f"{chain}: {f}", elements=n, share=round(a / n, 6))
        cap = CAP_LN if chain == "LayerNorm" else CAP_RMS
        assert a / n <= cap, f"{chain}, family {f}: {a / n:.3%} of the elements have two different bounds (cap {cap:.1%}): change the family"
    kinds, errors = {}, []
    for (kind, case), (a, n, cap) in groups.items():
        k = kinds.setdefault(kind, [1.0, 0.0, 0])
        k[0], k[1], k[2] = min(k[0], a / n), max(k[1], a / n), k[2] + 1
        if a / n > cap:
            errors.append(f"{kind} {case}: {a} of {n} elements ({a / n:.3%}) have two different bounds (cap {cap:.1%}): change the family")
    for kind, (lo_, hi_, n) in kinds.items():
        rec("ambiguity", kind, cases=n, min_share=round(lo_, 6), max_share=round(hi_, 6))
    assert not errors, "\n".join(errors)


# ---------------------------------------------------------------------------------------------------------- 3. mutants are rejected
def rms_model(x, w, eps, drop_eps=False, eps_after=False, eps_fixed=None, div=None, no_inner=False, skip_last_chunk=False):
    """the kernel's chain in fp32 at ONE rstd (torch's sum order), with the switches of the wrong variants"""
    xf = x.float()
    sq = xf * xf
    if skip_last_chunk:
        sq = sq.clone()
        sq[..., -8:] = 0.0
    ms = sq.sum(-1, keepdim=True) / float(div or x.shape[-1])
    e = torch.tensor(R.c32(eps if eps_fixed is None else eps_fixed), dtype=torch.float32)
    if drop_eps:
        r = 1.0 / torch.sqrt(ms)
    elif eps_after:
        r = 1.0 / (torch.sqrt(ms) + e)
    else:
        r = 1.0 / torch.sqrt(ms + e)
    inner = xf * r
    return (w.float() * (inner if no_inner else R.rb(inner))).to(BF16)


def rms_case(H, eps, T=9):
    x, fam = R.rms_rows(T, H, R.RMS_FINITE, 0, seed=3)
    w = R.rms_weight(H, 1)
    lo, hi, _ = R.rms_bounds(x, w, eps)
    return x, fam, w, lo, hi


def n_out(got, lo, hi, rows):
    return int(R.outside(got[rows], lo[rows], hi[rows]).sum())


@pytest.mark.parametrize("H", [1016, 4104])
def test_the_model_passes_and_rms_mutants_fail(H):
    for eps in (1e-6, 1.0):
        x, fam, w, lo, hi = rms_case(H, eps)
        every = torch.ones(len(fam), dtype=torch.bool)
        assert n_out(rms_model(x, w, eps), lo, hi, every) == 0, "the fp32 model itself must lie inside"
    x, fam, w, lo, hi = rms_case(H, 1e-6)
    small = rows_of(fam, "2^-10", "2^-12")
    for name in ("2^-10", "2^-12"):
        assert n_out(rms_model(x, w, 1e-6, drop_eps=True), lo, hi, rows_of(fam, name)) > 0, f"eps dropped, rows {name}"
        assert n_out(rms_model(x, w, 1e-6, eps_after=True), lo, hi, rows_of(fam, name)) > 0, f"eps after the square root, rows {name}"
    assert n_out(rms_model(x, w, 1e-6, drop_eps=True), lo, hi, rows_of(fam, "2^0")) == 0, "at unit scale eps cannot be seen (why the rows are there)"
    assert small.sum() == 2
    unit = rows_of(fam, "2^0")
    grid = 512 * (2 if H <= 1024 else 16)
    assert n_out(rms_model(x, w, 1e-6, div=grid), lo, hi, unit) > 0, "division by the chunk grid instead of H"
    assert n_out(rms_model(x, w, 1e-6, no_inner=True), lo, hi, unit) > 0, "inner bf16(x * r) rounding dropped"
    assert n_out(rms_model(x, w, 1e-6, skip_last_chunk=True), lo, hi, rows_of(fam, "onehot_last")) > 0, "last 16-byte chunk left out of the sum"
    x, fam, w, lo, hi = rms_case(H, 1.0)
    for name in R.RMS_SCALES:
        if name not in ("2^20", "2^50"):         # (ms >> 1 hides any eps)
            assert n_out(rms_model(x, w, 1.0, eps_fixed=1e-6), lo, hi, rows_of(fam, name)) > 0, f"eps hard-coded to 1e-6, eps = 1.0, rows {name}"


def test_expert_weight_mutant_fails():
    for c, lo, hi, nan_rows in rms_all():
        if c.expert is None or c.T < 3 or c.H < 1016 or c.eps != 1e-6:
            continue
        e = c.expert.bool() & ~rows_of(c.fam, "zero", *R.RMS_SPECIAL)
        if not bool(e.any()):
            continue
        assert n_out(rms_model(c.x, c.w, c.eps), lo, hi, e) > 0, f"{c.kernel} H={c.H}: gen norm weight not selected for expert rows"
        assert n_out(rms_model(c.x, c.w, c.eps), lo, hi, ~c.expert.bool() & ~nan_rows) == 0


def rope_model(c, gen=None, flip_rot=False, same_half=False, no_expert=False):
    """norm_rope_pair in fp32 at one rstd for the q heads of a qkv case, with the switches of the wrong variants"""
    gen = c.gen if gen is None else gen
    seg, slot, pos = R.qkv_layout(c.T)
    cos, sin = R.rope_table(c.hd, R.ROPE_ROWS)
    qn, kn, qg, kg = R.qkv_weights(c.hd)
    e = torch.zeros(c.T, dtype=torch.bool) if (c.expert is None or no_expert) else c.expert.bool()
    w = torch.where(e[:, None, None], qg[None, None, :], qn[None, None, :])
    cs, sn = cos[pos.long()][:, None, :], sin[pos.long()][:, None, :]
    if same_half:
        h = c.hd // 2
        cs, sn = torch.cat((cs[..., :h], cs[..., :h]), -1), torch.cat((sn[..., :h], sn[..., :h]), -1)
    x = c.x[:, :R.NQ]
    xf = x.float()
    r = 1.0 / torch.sqrt((xf * xf).sum(-1, keepdim=True) / float(c.hd) + torch.tensor(R.c32(c.eps)))
    t1, t2 = R.rope_terms(x, w, cs, sn, r, gen)
    return (t1 - t2 if flip_rot else t1 + t2).to(BF16)


def test_the_model_passes_and_rope_mutants_fail():
    seen = set()
    for c, q_lo, q_hi, *_ in qkv_all():
        if c.T < 11:
            continue
        what = f"hd={c.hd} T={c.T} gen={c.gen} eps={c.eps}"
        count = lambda got: int(R.outside(got, q_lo, q_hi).sum())
        assert count(rope_model(c)) == 0, "the fp32 model itself must lie inside: " + what
        assert count(rope_model(c, gen=not c.gen)) > 0, "und and gen chains swapped: " + what
        assert count(rope_model(c, flip_rot=True)) > 0, "rotate_half sign flipped: " + what
        assert count(rope_model(c, same_half=True)) > 0, "cos / sin read at d for both halves: " + what
        if c.gen:
            assert count(rope_model(c, no_expert=True)) > 0, "gen norm weight not selected for expert rows: " + what
        seen.add((c.hd, c.gen))
    assert len(seen) == 4


def ln_model(x, w, b, eps, raw_moment=False):
    mean, d, _ = R.ln_parts(x)
    q = (x.float() * x.float() if raw_moment else d * d).sum(-1, keepdim=True) / float(x.shape[-1])
    r = 1.0 / torch.sqrt(q + torch.tensor(R.c32(eps)))
    return R.ln_chain(d, w[None, :], b[None, :], r)


def test_the_model_passes_and_layernorm_mutant_fails():
    n = 0
    for c, lo, hi in ln_all():
        assert not bool(R.outside(ln_model(c.x, c.w, c.b, c.eps), lo, hi).any()), f"the fp32 model itself must lie inside: {c.kernel} H={c.H}"
        rows = torch.tensor([k[1] == "mean200" for k in c.fam])
        if c.H >= 1024 and bool(rows.any()):
            bad = ln_model(c.x, c.w, c.b, c.eps, raw_moment=True)
            assert int(R.outside(bad[rows], lo[rows], hi[rows]).sum()) > 0, f"variance without subtracting the mean: {c.kernel} H={c.H} eps={c.eps}"
            n += 1
    assert n >= 6
