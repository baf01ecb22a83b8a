"""ContinuousBatcher(paged=True, share_prefixes=True): requests with the same images share their KV pages (serving._prefill_shared,
kvcache.PagedCache.retain_prefix / adopt_prefix, prefix.py).  The yardstick of every test is the SAME batcher with the option off, with
logprobs=True: answers equal, log-probabilities equal bit for bit - sharing at chunk boundaries is exact, so there is no tolerance.
Tiny config (hd 128), ToyTokenizer; at vit_side 8 / patch 14 a 112 x 112 image is 64 patches + 2 markers = 66 context tokens, which the
tests assert before they rely on it: four images are a prefix of 264 tokens (one shared full page + a tail), two are 132 (a tail only).

What "exact" rests on, and how the request orders below are chosen.  A row's bits do not depend on what else is in its batch as long as
its GEMMs stay in one kernel family: up to 64 rows a GEMM runs on the weight-streaming kernels, above on the tiled
ones, and the two sum K in different orders.  A 448 x 448 image is 1024 patch rows, tiled however it is grouped; the tiny ViT's image is
64 rows, so alone it is on one side of that line and in a batched admission of two on the other.  Sharing changes who takes part in a
pass, so at THIS size a group of requests on one image would compare a 64-row ViT pass with the unshared run's 128-row one: measured,
equal answers, log-probabilities apart in the 4th digit (request 0 of such a group: -3.259399 against -3.258845).  So: in the tests
that follow the issue's request lists, neighbours in the queue never have the same number of images - every admission then is a
one-request pass in both runs (serving._prefill_many batches only groups with equal image counts) - and the leader / follower path
inside one batched admission is held to the same bit-for-bit yardstick by test_followers_inside_a_batched_admission, whose groups have
two leaders per image pass: 128 ViT rows shared, 256 unshared, the tiled kernels both ways."""
import pytest
import torch

from conftest import NEW_TOKEN_IDS

pytestmark = pytest.mark.gpu
P = 256


@pytest.fixture(scope="module")
def model(tiny_weights):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd.bagel import Bagel
    from unimedvl_amd.config import UniMedVLConfig
    cfg, sd, _, _ = tiny_weights
    return Bagel(UniMedVLConfig.from_dict(cfg), lambda n: sd[n], device="cuda", visual_gen=False)


def _images(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(3, 112, 112, generator=g).clamp(-1, 1) for _ in range(n)]


def _prompt(seed, n):
    g = torch.Generator().manual_seed(1000 + seed)
    return " ".join(str(int(v)) for v in torch.randint(5, 290, (n,), generator=g))


def _context_tokens(model, images, prompt=None):
    """the context length after `images` (and the prompt), by the host-side packing alone"""
    from oracle.toy_tokenizer import ToyTokenizer
    kvl, rope = [0], [0]
    for im in images:
        _, kvl, rope = model.prepare_vit_images(kvl, rope, [im], lambda x: x, NEW_TOKEN_IDS)
    if prompt is not None:
        _, kvl, rope = model.prepare_prompts(kvl, rope, [prompt], ToyTokenizer(NEW_TOKEN_IDS), NEW_TOKEN_IDS)
    return kvl[0]


class _Spy:
    """Around PagedCache.ensure_tokens: the shared pages a call is about to write (each would be a copy-on-write copy), and the peak
    of pages in use."""

    def __init__(self, monkeypatch):
        from unimedvl_amd.kvcache import PagedCache
        self.cow, self.peak = [], 0
        real = PagedCache.ensure_tokens
        spy = self

        def ensure_tokens(cache, need, *a, **kw):
            if cache.pool is not None:
                for s, n in enumerate(need):
                    pages = cache._pages(s)
                    if n > cache.lens[s]:
                        spy.cow += [(s, p) for p in pages[cache.lens[s] // P:(n + P - 1) // P] if cache.pool.refs[p] > 1]
            real(cache, need, *a, **kw)
            spy.peak = max(spy.peak, cache.pages_in_use())
        monkeypatch.setattr(PagedCache, "ensure_tokens", ensure_tokens)


def _watch_groups(monkeypatch):
    """the sizes of the admissions that were ONE batched pass for two or more requests (serving._prefill_many), both runs"""
    from unimedvl_amd.serving import ContinuousBatcher
    seen, real = [], ContinuousBatcher._prefill_many

    def many(self, slots, reqs):
        if len(reqs) > 1 and len({len(r.images) for r in reqs}) == 1:
            seen.append(len(reqs))
        return real(self, slots, reqs)
    monkeypatch.setattr(ContinuousBatcher, "_prefill_many", many)
    return seen


def _batcher(model, share, slots=3, check_every=4, use_graph=True, **kw):
    from oracle.toy_tokenizer import ToyTokenizer
    from unimedvl_amd.serving import ContinuousBatcher
    kw.setdefault("pool_pages", 64)
    return ContinuousBatcher(model, ToyTokenizer(NEW_TOKEN_IDS), NEW_TOKEN_IDS, lambda x: x, slots=slots, max_context=512, max_new_tokens=kw.pop("max_new_tokens", 8),
                             check_every=check_every, use_graph=use_graph, paged=True, logprobs=True, share_prefixes=share, **kw)


def _serve(srv, reqs):
    """reqs: (images, prompt, budget[, submit keywords]) -> [(answer, log-probabilities)] in request order"""
    rids = [srv.submit(r[0], r[1], max_new_tokens=r[2], **(r[3] if len(r) > 3 else {})) for r in reqs]
    got = srv.run()
    return [(got[r], srv.logprobs[r]) for r in rids]


def _assert_same(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], f"request {i}: answer {g[0]!r}, unshared {w[0]!r}"
        assert len(g[1]) == len(w[1]) and torch.equal(torch.tensor(g[1]).view(torch.int32), torch.tensor(w[1]).view(torch.int32)), \
            f"request {i}: log-probabilities {g[1]} differ from the unshared run's {w[1]}"


def _mixed_requests():
    """three requests on the same four images, two on the first two of them, one text-only, one on another image - in an order in which
    neighbours differ in their image count (module docstring)"""
    four, other = _images(4, seed=1), _images(1, seed=2)
    return [(four, _prompt(0, 5), 7), (four[:2], _prompt(3, 4), 5), (None, _prompt(5, 12), 6), (four, _prompt(1, 3), 6),
            (other, _prompt(6, 4), 7), (four[:2], _prompt(4, 6), 7), (four, _prompt(2, 9), 8)]


_MIXED = {}


def _mixed_runs(model, monkeypatch, slots, check_every, use_graph):
    key = (slots, check_every, use_graph)
    if key not in _MIXED:
        reqs = _mixed_requests()
        groups = _watch_groups(monkeypatch)
        off = _batcher(model, False, slots, check_every, use_graph)
        want = _serve(off, reqs)
        spy = _Spy(monkeypatch)
        on = _batcher(model, True, slots, check_every, use_graph)
        got = _serve(on, reqs)
        assert not groups, f"the test relies on one-request admissions (module docstring); batched: {groups}"
        _MIXED[key] = (reqs, off, want, on, got, list(spy.cow))
    return _MIXED[key]


@pytest.mark.parametrize("slots,check_every,use_graph", [(3, 4, True), (2, 5, False)])
def test_mixed_group_equals_the_unshared_batcher(model, monkeypatch, slots, check_every, use_graph):
    reqs, off, want, on, got, cow = _mixed_runs(model, monkeypatch, slots, check_every, use_graph)
    four = reqs[0][0]
    assert _context_tokens(model, four[:1]) == 66
    assert _context_tokens(model, four) == 264 > P, "one shared full page plus a tail"
    assert _context_tokens(model, four[:2]) == 132 < P, "a tail only"
    _assert_same(got, want)
    # the chain of the four images (its inner nodes serve the two-image requests) and the other image: 5 nodes, 5 ViT images
    assert on.stats["vit_images"] == 5, on.stats
    assert on.stats["prefix_hits"] >= 4 and on.stats["prefix_tokens_reused"] >= 2 * 264 + 2 * 132, on.stats
    assert on.stats["prefills"] == off.stats["prefills"] == len(reqs) and on.stats["tokens"] == off.stats["tokens"]
    assert "prefix_hits" not in off.stats and off.prefixes is None
    assert not cow, f"ensure_tokens met shared pages at a write position (segment, page): {cow}"


def test_end_state_accounting(model, monkeypatch):
    _, off, _, on, _, _ = _mixed_runs(model, monkeypatch, 3, 4, True)
    held = on.prefixes.pages_held()
    assert held > 0 and len(on.prefixes) >= 5 + len(_mixed_requests())
    assert held <= on.prefixes.max_pages == (64 - 1) // 4, "the default bound is a quarter of the pool"
    assert on.cache.pages_in_use() == off.cache.pages_in_use() + held
    on.drop_prefixes()
    assert len(on.prefixes) == 0 and on.cache.pages_in_use() == off.cache.pages_in_use()
    assert on.stats["prefix_evictions"] == 0


def test_identical_requests_under_per_request_sampling(model, monkeypatch):
    """one image, one prompt, five seeds: the prompt chunk hits, nothing but the first request is prefilled.  (A long text-only request
    keeps the second slot, so the five are admitted one by one in both runs.)"""
    from unimedvl_amd.sampling import SamplingParams
    im, prompt = _images(1, seed=3), _prompt(7, 6)
    reqs = [(im, prompt, 4, dict(sampling=SamplingParams(do_sample=True, temperature=1.5, top_k=40, seed=100 + i))) for i in range(5)]
    reqs.insert(1, (None, _prompt(9, 5), 24))
    reqs.append((im, _prompt(8, 6), 4, dict(sampling=SamplingParams(do_sample=True, temperature=0.7, seed=5))))
    kw = dict(slots=2, per_request_sampling=True, seed=9, max_new_tokens=24)
    groups = _watch_groups(monkeypatch)
    off = _batcher(model, False, **kw)
    want = _serve(off, reqs)
    on = _batcher(model, True, **kw)
    got = _serve(on, reqs)
    assert not groups, f"the test relies on one-request admissions (module docstring); batched: {groups}"
    _assert_same(got, want)
    assert len({g[0] for g in got if g is not got[1]}) > 1, "the seeds should give different answers, or the test compares nothing"
    n = _context_tokens(model, im, prompt)
    assert on.stats["vit_images"] == 1 and on.stats["prefix_hits"] == 5
    assert on.stats["prefix_tokens_reused"] == 4 * n + 66, (on.stats, n)


def test_persistence_and_poison(model, monkeypatch):
    """entries live across run() calls: a second run over the same images runs no ViT pass - and a repeat of the very first request,
    after others adopted its prefix and decoded behind it, still gets the first run's answer"""
    ims = _images(4, seed=4)
    f0, f1, f2, f3 = (ims, _prompt(10, 4), 4), (ims, _prompt(11, 5), 4), (ims, _prompt(12, 6), 4), (ims[:1], _prompt(20, 5), 12)
    first = [f0, f3, f1, f2]
    second = [f0, (ims[:3], _prompt(31, 3), 12), (ims, _prompt(30, 7), 4), f3, f2]
    groups = _watch_groups(monkeypatch)
    off = _batcher(model, False, slots=2, max_new_tokens=12)
    want1, want2 = _serve(off, first), _serve(off, second)
    on = _batcher(model, True, slots=2, max_new_tokens=12)
    got1 = _serve(on, first)
    assert on.stats["vit_images"] == 4
    hits = on.stats["prefix_hits"]
    assert hits == 3
    got2 = _serve(on, second)
    assert not groups, f"the test relies on one-request admissions (module docstring); batched: {groups}"
    _assert_same(got1, want1)
    _assert_same(got2, want2)
    assert got2[0] == got1[0] and got2[3] == got1[1] and got2[4] == got1[3]
    assert on.stats["vit_images"] == 4, "the second run computed an image again"
    assert on.stats["prefix_hits"] == hits + 5 and on.stats["prefills"] == 9


def test_prompt_ids_reach_the_penalties_on_a_prompt_hit(model, monkeypatch):
    """the text pass is skipped on a prompt-chunk hit, the prompt's ids are not: the repetition penalty's context set and the n-gram
    history are seeded from them"""
    im = _images(1, seed=5)
    prompt = "7 8 7 8 9 7 8 11 12 7"
    reqs = [(im, prompt, 8), (None, prompt, 24), (im, prompt, 8), (im, "7 8 9", 6), (im, prompt, 5), (None, prompt, 8)]
    kw = dict(slots=2, max_new_tokens=24, no_repeat_ngram_size=2, no_repeat_ngram_prompt=True, penalize_prompt=True, repetition_penalty=1.4)
    groups = _watch_groups(monkeypatch)
    off = _batcher(model, False, **kw)
    want = _serve(off, reqs)
    plain = _serve(_batcher(model, False, slots=2, max_new_tokens=24), reqs)
    on = _batcher(model, True, **kw)
    got = _serve(on, reqs)
    assert not groups, f"the test relies on one-request admissions (module docstring); batched: {groups}"
    _assert_same(got, want)
    assert [w[0] for w in want] != [p[0] for p in plain], "the penalties should change an answer, or the test compares nothing"
    assert on.stats["prefix_hits"] == 4 and on.stats["vit_images"] == 1


def test_small_pool_evicts_instead_of_failing(model, monkeypatch):
    """the pool is what the unshared run needs at its peak, not a page more: the sharing run completes in it - retained prefixes give
    way to every call that takes pages - with the same answers"""
    a, b, c = _images(4, seed=6), _images(4, seed=7), _images(2, seed=8)
    long = _prompt(44, 200)
    reqs = [(a, _prompt(40, 4), 7), (c, long, 8), (a, _prompt(41, 5), 6), (None, _prompt(46, 9), 5), (b, _prompt(42, 3), 8), (c, long, 6),
            (a, _prompt(43, 6), 5), (None, _prompt(47, 300), 4), (b, _prompt(45, 4), 7), (c, _prompt(48, 7), 6), (a, _prompt(40, 4), 7)]
    spy, groups = _Spy(monkeypatch), _watch_groups(monkeypatch)
    roomy = _batcher(model, False, slots=2, pool_pages=48)
    want = _serve(roomy, reqs)
    assert not groups, f"the test relies on one-request admissions (module docstring); batched: {groups}"
    pool = spy.peak + 1                       # page 0 is never handed out
    _assert_same(_serve(_batcher(model, False, slots=2, pool_pages=pool), reqs), want)
    with pytest.raises(RuntimeError, match="exhausted"):
        _serve(_batcher(model, False, slots=2, pool_pages=pool - 1), reqs)
    on = _batcher(model, True, slots=2, pool_pages=pool, prefix_cache_pages=64)
    got = _serve(on, reqs)
    _assert_same(got, want)
    assert on.stats["prefix_evictions"] > 0, on.stats       # (in a pool this tight entries rarely live long enough to be hit)
    assert not spy.cow


def test_followers_inside_a_batched_admission(model, monkeypatch):
    """four slots that fill and empty together: every admission is ONE batched pass per chunk.  Two leaders per image pass, followers
    that copy a leader's slot after the fourth image and after the prompt, and a hit on a chain that a batched pass retained."""
    x, y, z, w = (_images(4, seed=s) for s in (11, 12, 13, 14))
    reqs = [(x, _prompt(50, 6), 4), (x, _prompt(51, 6), 4), (y, _prompt(52, 6), 4), (y, _prompt(53, 6), 4),
            (z, _prompt(54, 6), 4), (w, _prompt(55, 6), 4), (z, _prompt(54, 6), 4), (x, _prompt(57, 6), 4)]
    groups = _watch_groups(monkeypatch)
    off = _batcher(model, False, slots=4)
    want = _serve(off, reqs)
    spy = _Spy(monkeypatch)
    on = _batcher(model, True, slots=4)
    got = _serve(on, reqs)
    assert groups == [4, 4, 4, 4], f"the test relies on two batched admissions of four in either run: {groups}"
    _assert_same(got, want)
    assert got[6] == got[4]
    assert on.stats["vit_images"] == 16 and on.stats["prefix_hits"] == 4, on.stats
    assert on.stats["prefix_tokens_reused"] == 3 * 264 + _context_tokens(model, z, _prompt(54, 6)), on.stats
    assert not spy.cow


@pytest.mark.parametrize("hd", [128, 64])
def test_adopted_contents_equal_the_source(hd):
    """the tail copy on the device (umv_beam_kv_copy, one launch per call): an adopted segment reads, through its own table row, the
    source's K and V^T bit for bit on the first n tokens; every page but the new tail pages keeps its bytes, and a new tail page
    changes in its first n % 256 tokens (rounded up to 8) only.  hd 128 is the tiny config's; 64 is the other width the copy serves."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from unimedvl_amd.kvcache import PagedCache
    layers, nkv = 2, 2
    g = torch.Generator().manual_seed(hd)
    for n in (8, 255, 300, 512 + 17):
        c = PagedCache(layers, pool_pages=20, max_context=2048)
        c.ensure_tokens([n, 0, 0, 200], nkv, hd, torch.device("cuda"))
        c.lens = [n, 0, 0, 200]
        for sl in c.pool.slabs:                  # every page of the pool holds its own random bits
            for t in (sl.k, sl.vt):
                t.view(torch.int16).copy_(torch.randint(-2 ** 15, 2 ** 15, t.shape, generator=g, dtype=torch.int16))
        before = [(sl.k.clone(), sl.vt.clone()) for sl in c.pool.slabs]
        src = [(c.view_segments(0, 1).packed_keys(l), c.view_segments(0, 1).packed_values(l)) for l in range(layers)]
        h = c.retain_prefix(0)
        c.adopt_prefix([(1, h), (2, c.live_prefix(0))])
        torch.cuda.synchronize()
        assert c.lens == [n, n, n, 200]
        full, t = n // P, n % P
        tails = [h.tail, c.pool.host_table[1][full], c.pool.host_table[2][full]]
        assert len(set(tails + c.pool.host_table[0] + c.pool.host_table[3])) == 3 + len(c.pool.host_table[0]) + 1
        assert c.pool.host_table[1][:full] == c.pool.host_table[2][:full] == c.pool.host_table[0][:full]
        for seg in (1, 2):
            v = c.view_segments(seg, seg + 1)
            for l in range(layers):
                assert torch.equal(v.packed_keys(l).view(torch.int16), src[l][0].view(torch.int16)), (n, seg, l, "K")
                assert torch.equal(v.packed_values(l).view(torch.int16), src[l][1].view(torch.int16)), (n, seg, l, "V^T")
        t8 = (t + 7) // 8 * 8
        old = c.pool.host_table[0][full]
        for (k0, v0), sl in zip(before, c.pool.slabs):
            exp_k, exp_v = k0.clone(), v0.clone()
            for pg in tails:
                exp_k[pg, :, :t8] = k0[old, :, :t8]
                exp_v[pg, :, :, :t8] = v0[old, :, :, :t8]
            assert torch.equal(sl.k.view(torch.int16), exp_k.view(torch.int16)), (n, "a K page changed that is not a new tail")
            assert torch.equal(sl.vt.view(torch.int16), exp_v.view(torch.int16)), (n, "a V^T page changed that is not a new tail")
        c.drop_prefix(h)
        for seg in range(4):
            c.release(seg)
        assert c.pages_in_use() == 0
