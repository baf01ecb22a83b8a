"""Forks of a paged KV cache (kvcache.PagedCache.snapshot) through the kernels, held to a dense reference.

  * kernels: one cache layer, 8 segments whose committed lengths sit on page edges; each took a decode horizon, wrote into it and was
    rewound (the gen_text pattern) before a snapshot.  Source and snapshot then append different causal chunks that cross page
    boundaries through umv_qkv_post.  Everything written through the table equals a plain KVSlab replay of the same calls, bit for
    bit; decode attention (split-KV, wave split) and prefill attention (library policy, TQ = 1 / 2, per-wave) on both sides equal the
    slab form bit for bit and exact fp64 attention on the shadow K / V within 2 bf16 ulp of the output range.  Every page starts as a
    finite poison value, so a read of a slot no one wrote on this side shows.
  * top of the pool: the largest pool the 32-bit page offsets of the PAGED prefill kernels allow (8191 pages of 256 KiB per operand
    at nkv 4, hd 128), one segment on the highest page ids.
  * engine: tiny model, decode in place with a horizon, rewind, snapshot; the source prefills a new prompt, the snapshot decodes, the
    source decodes - ids and logits equal the NaiveCache run bit for bit."""
import pytest
import torch

from test_attn_lazy_gpu import exact_attention, range_ulp
from test_paged_kv_gpu import _Tok, _tiny_model

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
NQ, NKV, HD = 28, 4, 128
POISON = 1e4


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd import ops as o
    return o


class _Writer:
    """umv_qkv_post calls replayed on a paged cache layer and a dense KVSlab: random QKV rows, unit q / k norms, rope tables of
    bounded angles."""

    def __init__(self, ops, seed, max_pos):
        self.ops = ops
        self.g = torch.Generator(device="cuda").manual_seed(seed)
        ang = torch.rand(max_pos, HD, generator=self.g, device="cuda") * 6.2831853
        self.cos, self.sin = ang.cos().to(BF16), ang.sin().to(BF16)
        self.w = torch.ones(HD, dtype=BF16, device="cuda")

    def write(self, targets, spans):
        """spans: per segment (lo, hi) - keys lo .. hi-1 appended to every slab in `targets`; returns q [T, NQ, HD]"""
        seg = torch.cat([torch.full((hi - lo,), s, dtype=torch.int32) for s, (lo, hi) in enumerate(spans)]).cuda()
        slot = torch.cat([torch.arange(lo, hi, dtype=torch.int32) for lo, hi in spans]).cuda()
        T = slot.numel()
        qkv = torch.randn(T, (NQ + 2 * NKV) * HD, generator=self.g, device="cuda").to(BF16)
        outs = []
        for slab in targets:
            q = torch.zeros(T, NQ, HD, dtype=BF16, device="cuda")
            self.ops.qkv_post(qkv, q, slab, seg, slot, slot, NQ, NKV, HD, 1e-6, self.w, self.w, cos_tab=self.cos, sin_tab=self.sin)
            outs.append(q)
        for q in outs[1:]:
            assert torch.equal(q, outs[0])
        return outs[0]


def _poisoned_slab(ops, nseg, cap):
    s = ops.KVSlab(nseg, NKV, cap, HD, "cuda")
    s.k.fill_(POISON)
    s.vt.fill_(POISON)
    return s


def _shadow(slab, lens):
    """per segment K / V [L, nkv, hd] of a dense slab: what the cache logically holds"""
    return ([slab.k[s, :, :n].transpose(0, 1) for s, n in enumerate(lens)],
            [slab.vt[s, :, :, :n].permute(2, 0, 1) for s, n in enumerate(lens)])


def _check_kv(cache, slab, name):
    ks, vs = _shadow(slab, cache.lens)
    got_k, got_v = cache.packed_keys(0), cache.packed_values(0)
    off = 0
    for s, (k, v) in enumerate(zip(ks, vs)):
        n = k.shape[0]
        pages = cache.pool.host_table[s]
        assert torch.equal(got_k[off:off + n], k), f"{name} segment {s}: K through the table != slab (pages {pages})"
        assert torch.equal(got_v[off:off + n], v), f"{name} segment {s}: V through the table != slab (pages {pages})"
        off += n


def _check_attention(ops, cache, slab, q_chunk, qlens, name):
    """decode and prefill attention through the table: == slab form, within 2 bf16 ulp of fp64 on the shadow, finite"""
    from unimedvl_amd import _lib as L
    lens = cache.lens
    nseg = len(lens)
    ks, vs = _shadow(slab, lens)
    kvl = torch.tensor(lens, dtype=torch.int32).cuda()
    ps = cache.slabs[0]

    def held(out, ref_out, ref64, what):
        assert torch.isfinite(out.float()).all(), f"{name} {what}: non-finite output"
        assert torch.equal(out, ref_out), f"{name} {what}: paged != slab in {(out != ref_out).sum().item()} elements"
        err, ulp = float((out.double() - ref64).abs().max()), range_ulp(ref64)
        assert err <= 2 * ulp, f"{name} {what}: max error {err:.4g} > 2 ulp of the output range ({ulp:.4g})"

    qd = torch.randn(nseg, NQ, HD, generator=torch.Generator(device="cuda").manual_seed(sum(lens)), device="cuda").to(BF16)
    ref64 = exact_attention(qd, ks, vs, [1] * nseg, True)
    cu = torch.arange(nseg + 1, dtype=torch.int32).cuda()
    for nsplit in (1, 4, 12):
        ws = ops.attn_workspace(nseg, NQ, HD, 1, nsplit, "cuda") if nsplit > 1 else None
        for wave_split in (0, 2):
            outs = []
            for sl in (ps, slab):
                out = torch.full_like(qd, float("nan"))
                ops.attention(qd, out, sl, cu, kvl, NQ, NKV, HD, True, 1, max(lens), nsplit=nsplit, workspace=ws, wave_split=wave_split)
                outs.append(out)
            held(outs[0], outs[1], ref64, f"decode nsplit {nsplit} wave_split {wave_split}")

    ref64 = exact_attention(q_chunk, ks, vs, qlens, True)
    cu = torch.tensor([0] + torch.tensor(qlens).cumsum(0).tolist(), dtype=torch.int32).cuda()
    for variant in (0, L.ATTN_FORCE | L.ATTN_TQ1, L.ATTN_FORCE | L.ATTN_TQ2, L.ATTN_FORCE | L.ATTN_STREAM):
        outs = []
        for sl in (ps, slab):
            out = torch.full_like(q_chunk, float("nan"))
            ops.attention(q_chunk, out, sl, cu, kvl, NQ, NKV, HD, True, max(qlens), max(lens), variant=variant)
            outs.append(out)
        held(outs[0], outs[1], ref64, f"prefill variant {variant:#x}")


def test_forks_through_the_kernels_against_fp64(ops):
    from unimedvl_amd.kvcache import PagedCache
    ctx = [1, 255, 256, 257, 511, 512, 513, 1000]          # committed lengths at page edges
    horizon = [300, 21, 260, 30, 1, 300, 21, 100]          # pages taken past them (a decode's), partly written, then rewound
    written = [21, 21, 21, 30, 1, 21, 21, 24]
    qa = [300, 20, 260, 300, 40, 260, 520, 60]             # the source's chunk, the snapshot's: each crosses a page boundary
    qb = [260, 3, 300, 256, 2, 257, 260, 30]
    nseg, cap = len(ctx), 1792
    for n, h, w, a, b in zip(ctx, horizon, written, qa, qb):
        assert w <= h and (n // 256 != (n + a - 1) // 256) and (n // 256 != (n + b - 1) // 256)
    src = PagedCache(1, pool_pages=160, max_context=2048)
    src.ensure_tokens([0] * nseg, NKV, HD, "cuda")
    for sl in src.pool.slabs:
        sl.k.fill_(POISON)
        sl.vt.fill_(POISON)
    wr = _Writer(ops, 5, cap)
    ref_src = _poisoned_slab(ops, nseg, cap)
    # context + a decode horizon written in place, then the committed length put back (inferencer.gen_text)
    src.ensure_tokens([n + h for n, h in zip(ctx, horizon)], NKV, HD, "cuda")
    wr.write([src.slabs[0], ref_src], [(0, n + w) for n, w in zip(ctx, written)])
    src.lens = list(ctx)
    snap = src.snapshot()
    ref_snap = _poisoned_slab(ops, nseg, cap)
    ref_snap.k.copy_(ref_src.k)
    ref_snap.vt.copy_(ref_src.vt)
    # the source appends chunk A, then the snapshot appends chunk B
    src.ensure_tokens([n + a for n, a in zip(ctx, qa)], NKV, HD, "cuda")
    q_a = wr.write([src.slabs[0], ref_src], [(n, n + a) for n, a in zip(ctx, qa)])
    src.lens = [n + a for n, a in zip(ctx, qa)]
    snap.ensure_tokens([n + b for n, b in zip(ctx, qb)], NKV, HD, "cuda")
    q_b = wr.write([snap.slabs[0], ref_snap], [(n, n + b) for n, b in zip(ctx, qb)])
    snap.lens = [n + b for n, b in zip(ctx, qb)]
    torch.cuda.synchronize()
    _check_kv(src, ref_src, "source")
    _check_kv(snap, ref_snap, "snapshot")
    _check_attention(ops, src, ref_src, q_a, qa, "source")
    _check_attention(ops, snap, ref_snap, q_b, qb, "snapshot")
    # the snapshot took the prefix pages only; after both appends the two sides share the full pages of the prefix and nothing else
    for s in range(nseg):
        shared = set(src.pool.host_table[s]) & set(snap.pool.host_table[s])
        assert len(shared) == ctx[s] // 256, f"segment {s}: source and snapshot share pages {sorted(shared)}, only full prefix pages may stay shared"
    for s in range(nseg):
        snap.release(s)
        src.release(s)
    assert src.pages_in_use() == 0


def test_top_of_the_largest_pool(ops):
    """8191 pages (2 GiB less one page per operand): one segment on pages 8190, 8189, ..., the next below it - umv_qkv_post writes,
    the PAGED prefill kernel of the library's policy and decode attention reach the last bytes under the 32-bit offset limit"""
    from unimedvl_amd.kvcache import PagedCache
    c = PagedCache(1, pool_pages=8191, max_context=2048)
    c.ensure_tokens([0, 0], NKV, HD, "cuda")
    for sl in c.pool.slabs:
        sl.k.fill_(POISON)
        sl.vt.fill_(POISON)
    c.pool.free.reverse()                                  # hand out the highest page ids first
    lens = [1300, 300]
    c.ensure_tokens(lens, NKV, HD, "cuda")
    assert c.pool.host_table == [list(range(8190, 8184, -1)), [8184, 8183]]
    assert c.pool.table[0, :6].tolist() == list(range(8190, 8184, -1))
    wr = _Writer(ops, 6, 2048)
    ref = _poisoned_slab(ops, 2, 1312)
    q = wr.write([c.slabs[0], ref], [(0, n) for n in lens])
    c.lens = list(lens)
    torch.cuda.synchronize()
    _check_kv(c, ref, "top of the pool")
    ks, vs = _shadow(ref, lens)
    kvl = torch.tensor(lens, dtype=torch.int32).cuda()
    cu = torch.tensor([0, 1300, 1600], dtype=torch.int32).cuda()
    ref64 = exact_attention(q, ks, vs, lens, True)
    out = torch.full_like(q, float("nan"))
    ops.attention(q, out, c.slabs[0], cu, kvl, NQ, NKV, HD, True, max(lens), max(lens))
    slab_out = torch.full_like(q, float("nan"))
    ops.attention(q, slab_out, ref, cu, kvl, NQ, NKV, HD, True, max(lens), max(lens))
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out, slab_out), "paged prefill at the top of the pool differs from the slab form"
    assert float((out.double() - ref64).abs().max()) <= 2 * range_ulp(ref64)
    qd = q[[1299, 1599]].contiguous()
    ref64 = exact_attention(qd, ks, vs, [1, 1], True)
    ws = ops.attn_workspace(2, NQ, HD, 1, 4, "cuda")
    out = torch.full_like(qd, float("nan"))
    ops.attention(qd, out, c.slabs[0], torch.arange(3, dtype=torch.int32).cuda(), kvl, NQ, NKV, HD, True, 1, max(lens), nsplit=4, workspace=ws)
    assert torch.isfinite(out.float()).all()
    assert float((out.double() - ref64).abs().max()) <= 2 * range_ulp(ref64)
    del c, ref
    torch.cuda.empty_cache()


def test_engine_fork_after_an_in_place_decode(tiny_weights):
    """decode in place (pages for the horizon), rewind, snapshot; the source prefills a new prompt, the snapshot decodes, then the
    source decodes: the same ids and logits as on NaiveCache, whose snapshots copy the whole slab"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from conftest import NEW_TOKEN_IDS
    from unimedvl_amd.kvcache import NaiveCache, PagedCache
    cfg, model = _tiny_model(tiny_weights)
    g = torch.Generator().manual_seed(23)
    prompts = [torch.randint(0, 290, (n,), generator=g).tolist() for n in (248, 254, 298, 30, 10, 240)]
    tok = _Tok(prompts)

    def run(cache):
        res = []
        gi, kvl, rope = model.prepare_prompts([0] * 3, [0] * 3, ["0", "1", "2"], tok, NEW_TOKEN_IDS)
        cache = model.forward_cache_update_text(cache, **gi)
        assert list(cache.lens) == [250, 256, 300]
        lens0 = list(cache.lens)
        gs = model.prepare_start_tokens(kvl, rope, NEW_TOKEN_IDS)
        res.append(model.generate_text(past_key_values=cache, max_length=20, return_logits=True, **gs))
        cache.lens = lens0                                      # inferencer.gen_text puts the committed length back
        snap = cache.snapshot()
        gi, kvl2, rope2 = model.prepare_prompts(kvl, rope, ["3", "4", "5"], tok, NEW_TOKEN_IDS)
        cache = model.forward_cache_update_text(cache, **gi)
        gs = model.prepare_start_tokens(kvl, rope, NEW_TOKEN_IDS)
        res.append(model.generate_text(past_key_values=snap, max_length=20, return_logits=True, **gs))
        gs = model.prepare_start_tokens(kvl2, rope2, NEW_TOKEN_IDS)
        res.append(model.generate_text(past_key_values=cache, max_length=20, return_logits=True, **gs))
        return res, cache, snap

    ref, _, _ = run(NaiveCache(cfg.layers))
    got, c, s = run(PagedCache(cfg.layers, pool_pages=64, max_context=2048))
    for what, (ids1, lg1), (ids2, lg2) in zip(("in-place decode", "snapshot decode", "source decode after the new prompt"), ref, got):
        assert torch.equal(ids1, ids2), f"{what}: ids differ from the NaiveCache run"
        assert all(torch.equal(a, b) for a, b in zip(lg1, lg2)), f"{what}: logits differ from the NaiveCache run"
    for seg in range(3):
        s.release(seg)
        c.release(seg)
    assert c.pages_in_use() == 0
