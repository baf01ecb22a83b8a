"""The RARE path of the prefill attention's lazy softmax (csrc/attention_prefill.hip::attn_softmax_lazy): the reference point moving on a
NON-EMPTY accumulator - O and l rescaled by alpha, the exponents already computed shifted by e - d, rows of one q-tile moving in
different blocks, rows that never see a key - which unit-scale randn scores never reach (the first block's maximum is ~2, nothing
later exceeds it by 8 log2 units).  A trained model takes that path all the time: peaked attention, sinks, learned q/k-norm gains.

Score distributions that force it (VERDICT r05 "next" #1):
  scale8 / scale32   q x 8 / x 32: peaked softmax, the maximum keeps moving by more than the trigger level
  ramp               keys ordered so that EVERY 32-key block raises every row's maximum by 16-32 log2 units
  outlier_last       one +40-nat key in the last block: one big rescale of a full accumulator
  outlier_first      the same key at position 1 (an attention sink): the reference is set once, far above everything after it
  mixed              the 16 rows of a q-tile mix flat rows (q = 0), ramp rows and peaked rows (per head; G = 7 dense tiles hold 2.3
                     tokens x 7 heads): a row moves only on its own trigger
  causal_short_kv    Lq > Lk under the bottom-right causal mask: the first Lq - Lk rows see no key at all (they stay "unset" to the end
                     and come out as zeros, flash-attn's convention), sharing tiles with rows that do

Every case runs on the shipped kernels (TQ = 1, TQ = 2, dense and whole-token tiles) through
umv_attn_args.variant, and is held to
  * EXACT attention in fp64 on the same bf16 inputs: max error <= 2 bf16 ulp of the output range, and no worse than 2x the error of
    the exact-running-maximum kernels (UMV_ATTN_VARIANT_EXACT) and of the per-wave kernel on the same inputs;
  * bit-identity among all lazy variants (a row's bits do not depend on its tile neighbours or on the tile packing), and between
    the counting (stats) instantiation and the plain one;
  * the device counters umv_attn_args.stats: the number of rescales of a non-empty accumulator is > 0 (the test cannot silently go
    flat again), resp. the number of first settings for the sink case;
  * determinism: the same call three times.
The same distributions go through attn_kernel (decode: one query row per segment, split-KV + combine) and its hd-512 form
(the VAE mid-block attention).  Reference semantics: qwen2_navit.py:605-614, siglip_navit.py:232-241 (flash_attn_varlen_func,
bottom-right causal: modeling_qwen2.py:369-372), autoencoder.py:50-62.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
LOG2E = 1.4426950408889634


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd import ops as o
    return o


def _variants():
    from unimedvl_amd import _lib as L
    F = L.ATTN_FORCE
    return L, {
        "tq1": F | L.ATTN_TQ1, "tq2": F | L.ATTN_TQ2, "tq1_whole": F | L.ATTN_TQ1 | L.ATTN_WHOLE_TOKENS,
        "tq2_whole": F | L.ATTN_TQ2 | L.ATTN_WHOLE_TOKENS,
        "exact_tq2": F | L.ATTN_TQ2 | L.ATTN_EXACT, "exact_tq1": F | L.ATTN_TQ1 | L.ATTN_EXACT, "stream": F | L.ATTN_STREAM,
    }


def make_case(dist, nq, nkv, hd, q_lens, k_lens, seed):
    """bf16 q [T, nq, hd] and per-segment K / V [Lk, nkv, hd] whose scores follow `dist`."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")
    T = sum(q_lens)
    q = rn(T, nq, hd)
    ks = [rn(lk, nkv, hd) for lk in k_lens]
    vs = [rn(lk, nkv, hd) for lk in k_lens]
    c = LOG2E / math.sqrt(hd)                        # exponent (log2 units) per unit of raw score
    if dist == "scale8":
        q *= 8
    elif dist == "scale32":
        q *= 32
    elif dist in ("ramp", "mixed"):
        # dimension 0 carries the ramp: k[i][0] = i, q[0] = a with a c in [0.5, 1.0): 16-32 log2 units per 32-key block
        slope = 0.5 + 0.5 * torch.rand(T, nq, generator=g, device="cuda")
        for k in ks:
            k[:, :, 0] = torch.arange(k.shape[0], device="cuda", dtype=torch.float32)[:, None]
        if dist == "ramp":
            q *= 0.05
            q[:, :, 0] = slope / c
        else:
            kind = torch.arange(nq, device="cuda") % 3                      # per head: 0 flat, 1 ramp, 2 peaked
            q[:, kind == 0] = 0
            q[:, kind == 1] *= 0.05
            q[:, kind == 1, 0] = (slope / c)[:, kind == 1]
            q[:, kind == 2] *= 8
            q[:, kind == 2, 0] = 0
    elif dist in ("outlier_last", "outlier_first"):
        q[:, :, 0] = 1.0
        for k in ks:
            k[:, :, 0] = 0
            pos = k.shape[0] - 3 if dist == "outlier_last" else 1
            k[pos, :, 0] = 40.0 * math.sqrt(hd)                           # +40 nats = +57.7 log2 units for every row
    elif dist != "unit":
        raise ValueError(dist)
    return q.to(BF16), [k.to(BF16) for k in ks], [v.to(BF16) for v in vs]


def exact_attention(q, ks, vs, q_lens, causal):
    """softmax(Q K^T / sqrt(d), bottom-right causal) V in fp64 on the bf16 inputs; rows without a visible key give zeros."""
    out = torch.empty(q.shape, dtype=torch.float64, device=q.device)
    t0 = 0
    for i, lq in enumerate(q_lens):
        k, v = ks[i].double(), vs[i].double()
        lk = k.shape[0]
        rep = q.shape[1] // k.shape[1]
        qf = q[t0:t0 + lq].double().transpose(0, 1)
        kf = k.transpose(0, 1).repeat_interleave(rep, dim=0)
        vf = v.transpose(0, 1).repeat_interleave(rep, dim=0)
        s = qf @ kf.transpose(1, 2) / math.sqrt(q.shape[-1])
        if causal:
            mask = torch.ones(lq, lk, dtype=torch.bool, device=q.device).tril(diagonal=lk - lq)
            s = s.masked_fill(~mask, float("-inf"))
        p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)
        out[t0:t0 + lq] = (p @ vf).transpose(0, 1)
        t0 += lq
    return out


def fill_slab(ops, ks, vs, nkv, hd, poison=1e4):
    cap = (max(k.shape[0] for k in ks) + 31) // 32 * 32
    slab = ops.KVSlab(len(ks), nkv, cap, hd, "cuda")
    slab.k.fill_(poison)          # a key / value beyond kv_len that is not masked wrecks the output
    slab.vt.fill_(poison)
    for i, (k, v) in enumerate(zip(ks, vs)):
        slab.k[i, :, :k.shape[0]] = k.transpose(0, 1)
        slab.vt[i, :, :, :k.shape[0]] = v.permute(1, 2, 0)
    return slab


def range_ulp(ref):
    """one bf16 ulp at the top of the output range"""
    return 2.0 ** (math.floor(math.log2(float(ref.abs().max().clamp_min(1e-30)))) - 7)


# (nq, nkv, hd): the LLM's GQA 28 / 4 x 128 (G = 7: dense tiles differ from whole-token tiles) and SigLIP's 16 x 72
HEADS = {128: (28, 4, 128), 72: (16, 16, 72)}
SHAPES = {
    "noncausal": ([300, 257, 64], [300 + 130, 257, 64 + 40], False),       # image spans over context + themselves
    "causal_ragged": ([200, 129, 77], [200 + 300, 129, 77 + 33], True),     # text after an image: bottom-right mask, ragged kv_len
}
DISTS = ["scale8", "scale32", "ramp", "outlier_last", "outlier_first", "mixed"]


def run_variants(ops, q, ks, vs, nq, nkv, hd, q_lens, causal, names):
    L, V = _variants()
    slab = fill_slab(ops, ks, vs, nkv, hd)
    cu = torch.tensor([0] + list(torch.tensor(q_lens).cumsum(0)), dtype=torch.int32).cuda()
    kvl = torch.tensor([k.shape[0] for k in ks], dtype=torch.int32).cuda()
    outs, stats = {}, {}
    for name in names:
        st = torch.zeros(2, dtype=torch.int32, device="cuda")
        runs = []
        for rep in range(3):
            out = torch.full(q.shape, float("nan"), dtype=BF16, device="cuda")
            ops.attention(q, out, slab, cu, kvl, nq, nkv, hd, causal, max(q_lens), int(kvl.max()), variant=V[name],
                          stats=st if (rep == 0 and name in ("tq1", "tq2")) else None)
            runs.append(out)
        torch.cuda.synchronize()
        assert torch.isfinite(runs[0].float()).all(), f"{name}: non-finite output"
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[1], runs[2]), f"{name}: the same call gave different bits (run 0 counted with stats)"
        outs[name] = runs[1]
        stats[name] = st.tolist()
    return outs, stats


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("hd", [128, 72])
def test_lazy_rescale_path_against_exact_attention(ops, hd, shape, dist):
    nq, nkv, _ = HEADS[hd]
    q_lens, k_lens, causal = SHAPES[shape]
    q, ks, vs = make_case(dist, nq, nkv, hd, q_lens, k_lens, seed=hd * 1000 + 100 * list(SHAPES).index(shape) + DISTS.index(dist))
    ref = exact_attention(q, ks, vs, q_lens, causal)
    lazy = ["tq1", "tq2", "tq1_whole", "tq2_whole"]
    outs, stats = run_variants(ops, q, ks, vs, nq, nkv, hd, q_lens, causal, lazy + ["exact_tq2", "exact_tq1", "stream"])
    # the rare path ran (on the kernels under test, counted on the device)
    for name in ("tq1", "tq2"):
        nonempty, first = stats[name]
        assert first > 0, (name, stats[name])
        if dist != "outlier_first":
            assert nonempty > 0, f"{name}: the reference never moved on a non-empty accumulator with '{dist}' scores - the test went flat"
    # one set of bits for every lazy variant (tile packing, tiles per wave, counting instantiation), one for the exact family
    for name in lazy[1:]:
        assert torch.equal(outs[name], outs["tq1"]), f"lazy variant {name} differs from tq1 in {(outs[name] != outs['tq1']).sum().item()} elements"
    assert torch.equal(outs["exact_tq2"], outs["stream"]) and torch.equal(outs["exact_tq1"], outs["stream"])
    # accuracy against exact fp64 attention, next to the exact-maximum kernels
    ulp = range_ulp(ref)
    err_lazy = (outs["tq1"].double() - ref).abs()
    err_exact = (outs["stream"].double() - ref).abs()
    assert float(err_lazy.max()) <= 2 * ulp, f"lazy max error {float(err_lazy.max()):.4g} > 2 ulp of the output range ({ulp:.4g})"
    assert float(err_lazy.max()) <= max(2.0 * float(err_exact.max()), ulp), (float(err_lazy.max()), float(err_exact.max()))
    assert float(err_lazy.mean()) <= 1.5 * float(err_exact.mean()) + 1e-6, (float(err_lazy.mean()), float(err_exact.mean()))


@pytest.mark.parametrize("hd", [128, 72])
def test_lazy_rows_that_see_no_key(ops, hd):
    """Lq > Lk under the causal mask: rows 0 .. Lq - Lk - 1 have every block fully masked (they never leave the 'unset' state: nm = 0,
    thr = -inf, l = 0 -> zeros), in the same q-tiles as rows that see 1, 2, ... keys; mixed score kinds on top."""
    nq, nkv, _ = HEADS[hd]
    q_lens, k_lens = [100, 70, 64], [70, 70, 40]
    q, ks, vs = make_case("mixed", nq, nkv, hd, q_lens, k_lens, seed=77 + hd)
    ref = exact_attention(q, ks, vs, q_lens, True)
    assert float(ref[:30].abs().max()) == 0.0 and float(ref[30].abs().max()) > 0
    outs, stats = run_variants(ops, q, ks, vs, nq, nkv, hd, q_lens, True, ["tq1", "tq2", "tq2_whole", "stream"])
    for name in ("tq1", "tq2", "tq2_whole", "stream"):
        assert float(outs[name][:30].float().abs().max()) == 0.0, f"{name}: a row without keys is not zero"
    assert torch.equal(outs["tq2"], outs["tq1"]) and torch.equal(outs["tq2_whole"], outs["tq1"])
    assert stats["tq2"][0] > 0
    ulp = range_ulp(ref)
    assert float((outs["tq1"].double() - ref).abs().max()) <= 2 * ulp
    assert float((outs["stream"].double() - ref).abs().max()) <= 2 * ulp


def test_lazy_kernels_at_bench_shapes(ops):
    """The shapes the bench legs run (8 x 1026 image spans; 8 x 1024 ViT patches), peaked and ramp scores: TQ = 2 by the library's own
    policy (variant = 0), counted."""
    from unimedvl_amd import _lib
    lib = _lib.load()
    for hd, L, dist in ((128, 1026, "scale8"), (128, 1026, "ramp"), (72, 1024, "scale8"), (72, 1024, "mixed")):
        nq, nkv, _ = HEADS[hd]
        assert lib.umv_attn_prefill_tq(8, nq, nkv, hd, L) == 2
        q, ks, vs = make_case(dist, nq, nkv, hd, [L] * 8, [L] * 8, seed=L + hd)
        slab = fill_slab(ops, ks, vs, nkv, hd)
        cu = torch.arange(0, 9 * L, L, dtype=torch.int32).cuda()
        kvl = torch.full((8,), L, dtype=torch.int32).cuda()
        st = torch.zeros(2, dtype=torch.int32, device="cuda")
        out = torch.zeros_like(q)
        ops.attention(q, out, slab, cu, kvl, nq, nkv, hd, False, L, L, stats=st)
        plain = torch.zeros_like(q)
        ops.attention(q, plain, slab, cu, kvl, nq, nkv, hd, False, L, L)
        assert torch.equal(out, plain), "the counting instantiation and the plain kernel differ"
        assert st[0].item() > 0
        ref = exact_attention(q[:L], ks[:1], vs[:1], [L], False)
        assert float((out[:L].double() - ref).abs().max()) <= 2 * range_ulp(ref)


def test_lazy_kernels_are_deterministic(ops):
    """Stress: 60 calls per variant on the shapes the bench legs run - image spans, the ViT at 8 and 32 images, a 4 096-token causal
    prefill, the guided flow pass - with peaked scores (the rare path fires in every wave), every CU busy and several waves per SIMD; every
    output equals the first.  (A paired-call form of the softmax - both q-tiles of a wave in one call - fails exactly this test, 39 of 39
    repeats, while it passes every small-shape parity case, and the SAME code passes at one wave per SIMD:
    profiles/r06_attn_pair_nondeterminism.txt.  It is not in the product build; the exact-maximum kernels are screened here too.)"""
    L_, V = _variants()
    cases = [(128, [1026] * 8, [1026] * 8, False), (72, [1024] * 8, [1024] * 8, False), (72, [1024] * 32, [1024] * 32, False),
             (128, [4096], [4096], True), (128, [258] * 12, [388] * 12, False), (128, [700, 513, 640, 1000], [1726, 553, 640, 1007], True)]
    for hd, q_lens, k_lens, causal in cases:
        nq, nkv, _ = HEADS[hd]
        q, ks, vs = make_case("scale8", nq, nkv, hd, q_lens, k_lens, seed=5)
        slab = fill_slab(ops, ks, vs, nkv, hd)
        cu = torch.tensor([0] + list(torch.tensor(q_lens).cumsum(0)), dtype=torch.int32).cuda()
        kvl = torch.tensor(k_lens, dtype=torch.int32).cuda()
        for name in ["tq2", "tq1", "exact_tq2"]:
            first, bad = None, 0
            for _ in range(60):
                out = torch.zeros_like(q)
                ops.attention(q, out, slab, cu, kvl, nq, nkv, hd, causal, max(q_lens), max(k_lens), variant=V[name])
                if first is None:
                    first = out
                else:
                    bad += int(not torch.equal(out, first))
            assert bad == 0, f"hd {hd} x {len(q_lens)} segments of {q_lens[0]} {name}: {bad} of 59 repeats differ from the first call"


@pytest.mark.parametrize("dist", ["scale32", "ramp", "outlier_last", "outlier_first", "mixed"])
@pytest.mark.parametrize("nsplit", [1, 4, 16])
def test_decode_attention_peaked_scores(ops, dist, nsplit):
    """attn_kernel as a decode step runs it (one query row per segment over 1060 / 777 / 33 cached keys, split-KV + attn_combine) on the
    same score distributions: the running-maximum softmax rescales in every block here, and the combine weights 2^(m_s - M) span the
    same dynamic range."""
    nq, nkv, hd = HEADS[128]
    q_lens, k_lens = [1, 1, 1], [1060, 777, 33]
    q, ks, vs = make_case(dist, nq, nkv, hd, q_lens, k_lens, seed=300 + nsplit)
    ref = exact_attention(q, ks, vs, q_lens, True)
    slab = fill_slab(ops, ks, vs, nkv, hd)
    cu = torch.tensor([0, 1, 2, 3], dtype=torch.int32).cuda()
    kvl = torch.tensor(k_lens, dtype=torch.int32).cuda()
    from unimedvl_amd import _lib
    ws = None
    if nsplit > 1:
        nbytes = _lib.load().umv_attn_workspace_bytes(3, nq, hd, 1, nsplit)
        ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.full(q.shape, float("nan"), dtype=BF16, device="cuda")
    ops.attention(q, out, slab, cu, kvl, nq, nkv, hd, True, 1, max(k_lens), nsplit=nsplit, workspace=ws)
    assert torch.isfinite(out.float()).all()
    assert float((out.double() - ref).abs().max()) <= 2 * range_ulp(ref)


@pytest.mark.parametrize("dist", ["scale8", "scale32", "ramp", "outlier_last"])
def test_vae_attention_hd512_peaked_scores(ops, dist):
    """attn_kernel<512>: the single-head attention of the VAE mid block (autoencoder.py:50-62) over 32 x 32 positions."""
    nq, nkv, hd = 1, 1, 512
    q_lens = k_lens = [1024, 256]
    q, ks, vs = make_case(dist, nq, nkv, hd, q_lens, k_lens, seed=41)
    ref = exact_attention(q, ks, vs, q_lens, False)
    slab = fill_slab(ops, ks, vs, nkv, hd)
    cu = torch.tensor([0, 1024, 1280], dtype=torch.int32).cuda()
    kvl = torch.tensor(k_lens, dtype=torch.int32).cuda()
    out = torch.full(q.shape, float("nan"), dtype=BF16, device="cuda")
    ops.attention(q, out, slab, cu, kvl, nq, nkv, hd, False, 1024, 1024)
    assert torch.isfinite(out.float()).all()
    assert float((out.double() - ref).abs().max()) <= 2 * range_ulp(ref)
