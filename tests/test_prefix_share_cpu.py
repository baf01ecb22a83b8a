"""Host side of prefix sharing (ContinuousBatcher(share_prefixes=True)) on CPU pools: PagedCache.retain_prefix / adopt_prefix /
drop_prefix - reference counts, every page back exactly once, refused calls take nothing, holders isolated from each other with no
copy-on-write -, pages_wanted against what ensure_tokens takes, the chunk keys, the hit / leader / follower partition, the table of
retained prefixes, and the keyword refusals.  (The batcher itself is a GPU test: tests/test_prefix_share_gpu.py.)"""
import inspect
import itertools

import pytest
import torch

from unimedvl_amd import ops
from unimedvl_amd.kvcache import PagedCache
from unimedvl_amd.prefix import PrefixTable, adopt_point, chunk_keys, image_key, plan_group

NKV, HD, LAYERS = 2, 8, 2
P = ops.KV_PAGE
LENGTHS = [0, 8, 255, 256, 257, 264, 512]


def _cache(nseg=3, pool_pages=16):
    c = PagedCache(LAYERS, pool_pages=pool_pages, max_context=2048)
    c.ensure_tokens([0] * nseg, NKV, HD, "cpu")
    return c


def _write(c, seg, lo, hi, val):
    """`val` + position (+ layer, head) into K / V^T of positions lo..hi-1 of a segment, through the host table"""
    if hi <= lo:
        return
    pos = torch.arange(lo, hi)
    pg = torch.tensor(c.pool.host_table[c._seg0 + seg])[pos // P]
    for l, sl in enumerate(c.slabs):
        for h in range(NKV):
            v = (val + pos + 7 * l + 3 * h).to(sl.k.dtype)
            sl.k[pg, h, pos % P, :] = v[:, None]
            sl.vt[pg, h, :, pos % P] = -v[:, None]


def _logical(c, seg):
    v = c.view_segments(seg, seg + 1)
    return [(v.packed_keys(l), v.packed_values(l)) for l in range(LAYERS)]


def _same(a, b):
    return all((x is None and y is None) or (torch.equal(x, y)) for la, lb in zip(a, b) for x, y in zip(la, lb))


def _prefill(c, seg, n, val=0):
    need = list(c.lens)
    need[seg] = n
    c.ensure_tokens(need, NKV, HD, "cpu")
    _write(c, seg, 0, n, val)
    c.lens[seg] = n


def _pool_state(c):
    return list(c.pool.refs), list(c.pool.free), [list(p) for p in c.pool.host_table], c.pool.table.clone(), list(c.lens)


def _unchanged(a, b):
    return a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and torch.equal(a[3], b[3]) and a[4] == b[4]


@pytest.mark.parametrize("n", LENGTHS)
def test_retain_adopt_drop_in_every_order(n):
    """source in segment 0, one retained handle, two adopters; the four holders let go in each of the 24 orders.  Reference counts are
    the holder counts, tails are private, every page comes back exactly once."""
    full, tail = n // P, int(n % P != 0)
    for order in itertools.permutations(("src", "a1", "a2", "handle")):
        c = _cache()
        _prefill(c, 0, n, val=10)
        assert c.pages_in_use() == full + tail
        src = _logical(c, 0)
        h = c.retain_prefix(0)
        assert h.n == n and len(h.full) == full and (h.tail is not None) == bool(tail) and h.owned
        assert c.pages_in_use() == full + 2 * tail
        assert all(c.pool.refs[p] == 2 for p in h.full) and (not tail or c.pool.refs[h.tail] == 1)
        c.adopt_prefix(1, h)
        c.adopt_prefix([(2, h)])
        assert c.lens == [n, n, n] and c.pages_in_use() == full + 4 * tail
        assert all(c.pool.refs[p] == 4 for p in h.full)
        for seg in (1, 2):
            pages = c.pool.host_table[seg]
            assert pages[:full] == h.full and len(pages) == full + tail
            assert all(c.pool.refs[p] == 1 for p in pages[full:]) and (not tail or pages[full] not in (h.tail, c.pool.host_table[0][full]))
            row = c.pool.table[seg]
            assert row[:len(pages)].tolist() == pages and not row[len(pages):].any()
            assert _same(_logical(c, seg), src)
        holders = 4
        for who in order:
            if who == "handle":
                c.drop_prefix(h)
                c.drop_prefix(h)            # a second drop returns nothing twice
            else:
                c.release({"src": 0, "a1": 1, "a2": 2}[who])
            holders -= 1
            assert all(c.pool.refs[p] == holders for p in h.full)
            assert c.pages_in_use() == (full if holders else 0) + holders * tail
            for seg, name in ((0, "src"), (1, "a1"), (2, "a2")):      # the ones still held read what they read before
                if order.index(name) > order.index(who):
                    assert _same(_logical(c, seg), src)
        assert c.pages_in_use() == 0 and len(set(c.pool.free)) == len(c.pool.free) == c.pool.npages - 1
        assert not any(c.pool.refs)


@pytest.mark.parametrize("n", LENGTHS)
def test_adopt_after_the_source_is_gone_and_from_a_live_slot(n):
    c = _cache()
    _prefill(c, 0, n, val=40)
    src = _logical(c, 0)
    h = c.retain_prefix(0)
    c.release(0)
    _prefill(c, 0, 100, val=900)            # the freed pages are taken and rewritten by someone else
    c.adopt_prefix(1, h)
    assert _same(_logical(c, 1), src)
    c.adopt_prefix(2, c.live_prefix(1))     # a follower copies a live slot: nothing is retained in between
    assert _same(_logical(c, 2), src) and c.lens[2] == n
    c.drop_prefix(c.live_prefix(1))         # owns nothing: nothing happens
    assert _same(_logical(c, 1), src)
    c.drop_prefix(h)
    assert _same(_logical(c, 1), src) and _same(_logical(c, 2), src)
    for seg in range(3):
        c.release(seg)
    assert c.pages_in_use() == 0 and not any(c.pool.refs)


def test_refused_calls_take_nothing():
    c = _cache(nseg=4, pool_pages=5)        # 4 usable pages
    _prefill(c, 0, 300)                     # 2 pages
    h = c.retain_prefix(0)                  # + 1 tail
    c.adopt_prefix(1, h)                    # + 1 tail: the pool is full
    before = _pool_state(c)
    with pytest.raises(RuntimeError, match="exhausted"):
        c.retain_prefix(0)
    with pytest.raises(RuntimeError, match="exhausted"):
        c.retain_prefix([1, 0])
    with pytest.raises(RuntimeError, match="exhausted"):
        c.adopt_prefix(2, h)
    with pytest.raises(RuntimeError, match="exhausted"):
        c.adopt_prefix([(2, h), (3, h)])
    with pytest.raises(ValueError, match="release it first"):
        c.adopt_prefix(1, h)                # the segment holds a context
    with pytest.raises(ValueError, match="twice"):
        c.adopt_prefix([(2, h), (2, h)])
    assert _unchanged(before, _pool_state(c))
    # a group is all or nothing too: room for one tail, two wanted
    c.release(1)
    before = _pool_state(c)
    with pytest.raises(RuntimeError, match="exhausted"):
        c.adopt_prefix([(2, h), (3, h)])
    assert _unchanged(before, _pool_state(c))
    c.adopt_prefix([(2, h)])
    # a prefix of full pages only needs no page: it fits a full pool
    c.release(2), c.release(0), c.drop_prefix(h)
    assert c.pages_in_use() == 0
    _prefill(c, 0, 4 * P)
    h = c.retain_prefix(0)
    c.adopt_prefix([(1, h), (2, h)])
    assert c.pages_in_use() == 4 and all(c.pool.refs[p] == 4 for p in h.full)
    short = PagedCache(1, pool_pages=8, max_context=256)
    short.pool, short.lens = c.pool, [0] * 4
    with pytest.raises(ValueError, match="reach"):
        short.adopt_prefix(3, h)            # beyond the adopter's page table


@pytest.mark.parametrize("n", [8, 255, 256, 300, 512, 520])
def test_holders_are_isolated_without_copy_on_write(n):
    """pattern in the source, an entry and two adopters; the source and both adopters append different tokens.  Each holder keeps its
    own logical K and V^T, the entry's tail stays as it was, no write position meets a shared page, and ensure_tokens takes exactly
    the pages growth needs - none for a copy-on-write."""
    c = _cache(pool_pages=24)
    _prefill(c, 0, n, val=5)
    prefix = _logical(c, 0)
    h = c.retain_prefix(0)
    c.adopt_prefix([(1, h), (2, h)])
    t = n % P
    tail0 = [(sl.k[h.tail, :, :t].clone(), sl.vt[h.tail, :, :, :t].clone()) for sl in c.slabs] if t else None
    grow = {0: 10, 1: 300, 2: 1}
    for seg, q in grow.items():
        need = list(c.lens)
        need[seg] = n + q
        used = c.pages_in_use()
        want = c.pages_wanted(need)
        assert want == (n + q + P - 1) // P - (n + P - 1) // P, "a holder of a prefix wants pages for growth only"
        c.ensure_tokens(need, NKV, HD, "cpu")
        assert c.pages_in_use() - used == want
        pages = c.pool.host_table[seg]
        shared = [(i, pages[i]) for i in range(n // P, (n + q + P - 1) // P) if c.pool.refs[pages[i]] != 1]
        assert not shared, f"segment {seg} writes (index, page) {shared}, shared with another holder"
        _write(c, seg, n, n + q, val=1000 * (seg + 1))
        c.lens[seg] = n + q
    for seg, q in grow.items():
        got = _logical(c, seg)
        for l in range(LAYERS):
            assert torch.equal(got[l][0][:n], prefix[l][0]) and torch.equal(got[l][1][:n], prefix[l][1]), f"segment {seg} lost its prefix"
            pos = torch.arange(n, n + q)
            for hd in range(NKV):
                want = (1000 * (seg + 1) + pos + 7 * l + 3 * hd).to(got[l][0].dtype)
                assert torch.equal(got[l][0][n:, hd, 0], want) and torch.equal(got[l][1][n:, hd, 0], -want), f"segment {seg} reads another's append"
    if t:
        for sl, (k0, v0) in zip(c.slabs, tail0):
            assert torch.equal(sl.k[h.tail, :, :t], k0) and torch.equal(sl.vt[h.tail, :, :, :t], v0), "the entry's tail changed"
    # a late adopter still gets the prefix, not what the others wrote behind it
    c.release(2)
    c.adopt_prefix(2, h)
    assert _same(_logical(c, 2), prefix)


def test_pages_wanted_is_what_ensure_tokens_takes():
    fresh = PagedCache(LAYERS, pool_pages=32, max_context=2048)
    assert fresh.pages_wanted([300, 0, 256]) == 2 + 0 + 1           # no pool yet: every page is new
    c = _cache(pool_pages=32)
    g = torch.Generator().manual_seed(3)
    snaps = []
    for step in range(60):
        cur = c if not snaps or step % 3 else snaps[step % len(snaps)]
        need = [min(2048, n + int(torch.randint(0, 400, (1,), generator=g))) if int(torch.randint(0, 2, (1,), generator=g)) else n
                for n in cur.lens]
        want, free = cur.pages_wanted(need), len(c.pool.free)
        if want > free:
            with pytest.raises(RuntimeError):
                cur.ensure_tokens(need, NKV, HD, "cpu")
            assert len(c.pool.free) == free
            for s in range(3):
                cur.release(s)
            continue
        cur.ensure_tokens(need, NKV, HD, "cpu")
        assert free - len(c.pool.free) == want, (step, need, want)
        cur.lens = [max(a, b) for a, b in zip(cur.lens, need)]
        if step % 7 == 2 and len(snaps) < 3:                       # shared pages: the copy-on-write part of the count
            snaps.append(c.snapshot())
        if step % 11 == 5:                                         # ... and a prefix held three ways
            c.release(2)
            c.adopt_prefix(2, c.live_prefix(0))
    with pytest.raises(ValueError, match="reach"):
        c.pages_wanted([4000, 0, 0])


def test_image_keys():
    from PIL import Image
    g = torch.Generator().manual_seed(0)
    t = torch.randn(3, 28, 42, generator=g)
    assert image_key(t) == image_key(t.clone()) and len(image_key(t)) == 16
    assert image_key(t) == image_key(t.permute(1, 0, 2).contiguous().permute(1, 0, 2)), "the key reads a contiguous copy"
    bit = t.clone()
    bit.view(torch.int32)[1, 2, 3] ^= 1
    assert image_key(bit) != image_key(t), "one bit"
    assert image_key(t.reshape(3, 42, 28)) != image_key(t), "same bytes, another shape"
    assert image_key(t.view(torch.int32)) != image_key(t), "same bytes, another dtype"
    assert image_key(t.to(torch.bfloat16)) == image_key(t.to(torch.bfloat16).clone())
    px = (torch.rand(20, 30, 3, generator=g) * 255).to(torch.uint8).numpy()
    im = Image.fromarray(px, "RGB")
    assert image_key(im) == image_key(Image.fromarray(px.copy(), "RGB"))
    px2 = px.copy()
    px2[4, 5, 1] ^= 1
    assert image_key(Image.fromarray(px2, "RGB")) != image_key(im)
    assert image_key(im.convert("L")) != image_key(im) and image_key(im.resize((10, 60))) != image_key(im)
    with pytest.raises(TypeError, match="image_keys"):
        image_key("a path")
    # chunk keys: images in order, then the prompt's packed ids; the caller's keys replace the digests and are not looked into
    a = chunk_keys([t, im], [300, 5, 6, 301])
    assert a == (("img", image_key(t)), ("img", image_key(im)), ("txt", (300, 5, 6, 301)))
    b = chunk_keys(["never hashed", object], [300, 5, 6, 301], image_keys=["study-1", ("series", 2)])
    assert b == (("img", "study-1"), ("img", ("series", 2)), ("txt", (300, 5, 6, 301)))
    assert chunk_keys([], [300, 301]) == (("txt", (300, 301)),)
    with pytest.raises(ValueError, match="image_keys"):
        chunk_keys([t], [300, 301], image_keys=[1, 2])


def _plan(chains, cached=()):
    cached = set(cached)
    states, leader = plan_group(chains, cached.__contains__)
    return ["".join(s[0] for s in st) for st in states], leader, [adopt_point(st) for st in states]


def test_leaders_followers_and_hits():
    A, B, C, D = ("img", "a"), ("img", "b"), ("img", "c"), ("img", "d")
    p, q, r = ("txt", (1,)), ("txt", (2,)), ("txt", (3,))
    # three requests on the same two images, different prompts: one leader per image, everyone leads its own prompt
    states, leader, at = _plan([(A, B, p), (A, B, q), (A, B, r)])
    assert states == ["lll", "ffl", "ffl"] and at == [-1, 1, 1]
    assert leader == [[None] * 3, [0, 0, None], [0, 0, None]]
    # identical requests: the prompt chunk is followed as well
    states, leader, at = _plan([(A, p), (A, p), (A, q)])
    assert states == ["ll", "ff", "fl"] and at == [-1, 1, 0] and leader[1] == [0, 0]
    # the leader diverges after the first image: the two that go on together get a leader of their own for the second
    states, leader, at = _plan([(A, C, p), (A, B, p), (A, B, q), (D, B, q)])
    assert states == ["lll", "fll", "ffl", "lll"] and at == [-1, 0, 1, -1]
    assert leader[2] == [0, 1, None] and leader[1] == [0, None, None]
    # the longest cached chain wins: one adoption at the deepest hit, also where an inner node is gone from the table
    states, leader, at = _plan([(A, B, p), (A, B, q), (A, q), (C, p)], cached=[(A,), (A, B), (A, B, p)])
    assert states == ["hhh", "hhl", "hl", "ll"] and at == [2, 1, 0, -1]
    states, leader, at = _plan([(A, B, p), (A, q)], cached=[(A, B)])
    assert states == ["hhl", "ll"] and at == [1, -1], "an inner node that was evicted is computed again by whoever needs it alone"
    # a cached head, then a shared new tail inside the group
    states, leader, at = _plan([(A, B, C, p), (A, B, C, q)], cached=[(A,)])
    assert states == ["hlll", "hffl"] and at == [0, 2] and leader[1] == [None, 0, 0, None]
    # an image key never meets a prompt key; different lengths are fine; an empty group is too
    states, _, _ = _plan([(("img", (1,)),), (("txt", (1,)),)])
    assert states == ["l", "l"]
    assert plan_group([], lambda key: False) == ([], [])
    # states always read hit* follow* lead*
    import random
    rng = random.Random(4)
    for _ in range(200):
        chains = [tuple(("img", rng.randrange(3)) for _ in range(rng.randrange(0, 4))) + (("txt", (rng.randrange(2),)),) for _ in range(5)]
        cached = {c[:i] for c in chains for i in range(1, len(c) + 1) if rng.random() < 0.3}
        states, leader, at = _plan(chains, cached)
        for s_, c, ld in zip(states, chains, leader):
            assert s_ == "h" * s_.count("h") + "f" * s_.count("f") + "l" * s_.count("l"), (chains, cached, states)
            for j, who in enumerate(ld):
                assert (who is not None) == (s_[j] == "f")
                if who is not None:
                    assert states[who][j] == "l" and chains[who][:j + 1] == c[:j + 1]
        led = [c[:j + 1] for s_, c in zip(states, chains) for j in range(len(c)) if s_[j] == "l"]
        assert len(led) == len(set(led)) and not set(led) & cached, "every new prefix is computed once"


def test_prefix_table_bound_lru_and_room():
    c = _cache(nseg=4, pool_pages=12)       # 11 usable pages
    stats = {}
    tab = PrefixTable(c, 4, stats)
    for seg, n in enumerate((300, 556, 100)):                    # a chain: 1 + tail, 2 + tail; and a stranger: tail only
        if seg == 1:
            c.adopt_prefix(1, c.live_prefix(0))
            c.ensure_tokens([300, 556, 0, 0], NKV, HD, "cpu")
            c.lens[1] = 556
        else:
            _prefill(c, seg, n)
    tab.put(("a",), c.retain_prefix(0), 1)
    tab.put(("a", "b"), c.retain_prefix(1), 2)
    assert tab.pages_held() == 4, "distinct pages: the chain's first page counts once, the two tails and the second page once each"
    tab.trim()
    assert len(tab) == 2 and stats["prefix_evictions"] == 0
    tab.put(("z",), c.retain_prefix(2), 1)
    assert tab.pages_held() == 5
    assert tab.get(("a", "b"))[1] == 2                           # touches ("a",) too: ("z",) is the least recently used now
    tab.trim()
    assert ("z",) not in tab and ("a",) in tab and ("a", "b") in tab and stats["prefix_evictions"] == 1
    for seg in range(3):
        c.release(seg)
    assert c.pages_in_use() == tab.pages_held() == 4
    # make_room: entries give way, least recently used first, until the call fits - and not one more
    tab.make_room(8, keep={("a",)})
    assert ("a", "b") not in tab and ("a",) in tab and len(c.pool.free) == 9
    tab.make_room(11)
    assert len(tab) == 0 and c.pages_in_use() == 0 and stats["prefix_evictions"] == 3
    tab.make_room(50)                                            # nothing left to evict: the caller's call fails on its own
    _prefill(c, 0, 10)
    tab.put(("k",), c.retain_prefix(0), 1)
    tab.clear()
    assert len(tab) == 0 and c.pages_in_use() == 1 and stats["prefix_evictions"] == 3, "clear() is no eviction"


def test_keywords_and_refusals():
    from unimedvl_amd.serving import ContinuousBatcher, MixedBatcher
    sig = inspect.signature(ContinuousBatcher.__init__).parameters
    for name, default in (("share_prefixes", False), ("prefix_cache_pages", None)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default is default
    assert "image_keys" in inspect.signature(ContinuousBatcher.submit).parameters
    assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(MixedBatcher.__init__).parameters.values())
    assert callable(ContinuousBatcher.drop_prefixes)
    with pytest.raises(ValueError, match="paged=True"):
        ContinuousBatcher(None, None, {}, None, share_prefixes=True)
    with pytest.raises(ValueError, match="paged=True"):
        ContinuousBatcher(None, None, {}, None, prefix_cache_pages=8)
    with pytest.raises(ValueError, match="paged=True"):
        MixedBatcher(None, None, None, {}, None, share_prefixes=True)
    with pytest.raises(ValueError, match="share_prefixes=True"):
        ContinuousBatcher(None, None, {}, None, paged=True, prefix_cache_pages=8)
