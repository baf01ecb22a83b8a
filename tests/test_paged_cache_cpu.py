"""Host logic of kvcache.PagedCache (the block-table KV cache) on CPU tensors: page accounting, the device table's
contents, release / re-use, reference-counted snapshots with copy-on-write of every shared page an append writes, segment views, the
pool bounds, and a seeded model-based driver that holds all of it to a dense shadow of every cache.
(The kernels that read the table are GPU tests: tests/test_paged_kv_gpu.py, tests/test_paged_forks_gpu.py.)"""
import random

import pytest
import torch

from unimedvl_amd import ops
from unimedvl_amd.kvcache import PagedCache

NKV, HD = 1, 8
P = ops.KV_PAGE


def _fill(c, seg, lo, hi, val):
    """write `val + position` into K / V^T of positions lo..hi-1 of a segment, through the table (what umv_qkv_post does on the device)"""
    for l, sl in enumerate(c.slabs):
        for pos in range(lo, hi):
            pg = int(sl.table[seg, pos // P])
            sl.k[pg, :, pos % P, :] = val + pos + 1000 * l
            sl.vt[pg, :, :, pos % P] = val + pos + 1000 * l


def test_pages_follow_the_context_and_come_back():
    c = PagedCache(2, pool_pages=12, max_context=2048)
    c.ensure_tokens([300, 10, 0], NKV, HD, "cpu")
    assert c.pages_in_use() == 2 + 1 + 0 and c.cap == 2048
    t = c.slabs[0].table
    assert t.shape == (3, 8) and len({int(t[0, 0]), int(t[0, 1]), int(t[1, 0])}) == 3 and 0 not in (int(t[0, 0]), int(t[0, 1]), int(t[1, 0]))
    c.lens = [300, 10, 0]
    c.ensure_tokens([300, 10, 0], NKV, HD, "cpu")               # nothing grows: nothing is taken
    assert c.pages_in_use() == 3
    c.ensure_tokens([513, 10, 256], NKV, HD, "cpu")             # 3 pages, 1 page, exactly one page
    assert c.pages_in_use() == 3 + 1 + 1
    with pytest.raises(ValueError):
        c.ensure_tokens([4000, 10, 256], NKV, HD, "cpu")        # beyond the table's reach
    with pytest.raises(RuntimeError):
        c.ensure_tokens([2048, 2048, 256], NKV, HD, "cpu")      # beyond the pool (11 usable pages)
    assert c.pages_in_use() == 5, "a refused request must not keep pages"
    used = c.pages_in_use()
    c.release(0)
    assert c.lens[0] == 0 and c.pages_in_use() < used
    c.release(1), c.release(2)
    assert c.pages_in_use() == 0
    c.ensure_tokens([8 * P, 3 * P, 0], NKV, HD, "cpu")          # every page of the pool can be taken again
    assert c.pages_in_use() == 11


def test_snapshot_shares_pages_and_copies_the_last_one_on_append():
    c = PagedCache(2, pool_pages=16, max_context=2048)
    c.ensure_tokens([300, 256], NKV, HD, "cpu")
    _fill(c, 0, 0, 300, 0.0), _fill(c, 1, 0, 256, 5000.0)
    c.lens = [300, 256]
    s = c.snapshot()
    assert c.pages_in_use() == 3 and s.lens == [300, 256]
    k0 = [c.packed_keys(l).clone() for l in range(2)]
    # the original appends: segment 0's half-filled last page is shared -> copied; segment 1 ends on a page boundary -> a fresh page
    c.ensure_tokens([310, 260], NKV, HD, "cpu")
    assert c.pages_in_use() == 3 + 1 + 1
    _fill(c, 0, 300, 310, 0.0), _fill(c, 1, 256, 260, 5000.0)
    c.lens = [310, 260]
    for l in range(2):
        assert torch.equal(s.packed_keys(l), k0[l]), "the snapshot must not see the original's appends"
        assert torch.equal(c.packed_keys(l)[:300], k0[l][:300]) and torch.equal(c.packed_values(l)[310:566], s.packed_values(l)[300:556])
    # the snapshot appends too: its last page of segment 0 is its own by now (the original left it), no further copy
    s.ensure_tokens([305, 256], NKV, HD, "cpu")
    assert c.pages_in_use() == 5
    _fill(s, 0, 300, 305, 9000.0)
    s.lens = [305, 256]
    assert torch.equal(c.packed_keys(0)[300:310, 0, 0], torch.arange(300, 310).float().to(c.packed_keys(0).dtype))
    # releasing both sides returns every page exactly once
    for seg in range(2):
        c.release(seg), s.release(seg)
    assert c.pages_in_use() == 0


def test_views_share_the_pool():
    c = PagedCache(1, pool_pages=10, max_context=1024)
    c.ensure_tokens([0, 0, 0], NKV, HD, "cpu")
    v = c.view_segments(1, 2)
    v.ensure_tokens([600], NKV, HD, "cpu")
    v.lens = [600]
    assert c.pages_in_use() == 3 and len(c.pool.host_table[1]) == 3 and c.pool.host_table[0] == []
    assert v.slabs[0].table.data_ptr() == c.slabs[0].table[1:2].data_ptr() and v.slabs[0].table.stride(0) == c.slabs[0].table.stride(0)
    c.lens[1] = v.lens[0]
    assert c.packed_keys(0).shape[0] == 600


def test_pool_larger_than_32_bit_offsets_is_refused():
    with pytest.raises(ValueError):
        c = PagedCache(1, pool_pages=9000, max_context=1024)
        c.ensure_tokens([1], 4, 128, "meta")


def test_pool_of_8191_pages_is_the_largest_accepted():
    """nkv 4, hd 128: a page is 256 KiB per operand, so 8191 pages stay below 2 GiB (the PAGED prefill kernels' 32-bit offsets), 8192 do not"""
    c = PagedCache(1, pool_pages=8191, max_context=1024)
    c.ensure_tokens([1], 4, 128, "meta")
    assert c.pool.npages == 8191 and c.pool.slabs[0].k.numel() * 2 == 8191 * 4 * P * 128 * 2 <= 2 ** 31 - 1
    with pytest.raises(ValueError):
        PagedCache(1, pool_pages=8192, max_context=1024).ensure_tokens([1], 4, 128, "meta")


# --- regressions: a snapshot taken while the source holds pages beyond its committed length (a decode horizon, a rewind)

def _tags(c, seg, lo, hi, val):
    """write `val` (+ the layer) into K / V^T of positions lo..hi-1 of a segment through the host table, vectorised"""
    pos = torch.arange(lo, hi)
    pg = torch.tensor(c.pool.host_table[c._seg0 + seg])[pos // P]
    for l, sl in enumerate(c.slabs):
        sl.k[pg, :, pos % P, :] = float(val + l)
        sl.vt[pg, :, :, pos % P] = float(val + l)


def _shared_pages_written(c, seg, lo, hi):
    """the pages behind positions lo..hi-1 of a segment that another cache still holds (refs > 1)"""
    pages = c.pool.host_table[c._seg0 + seg]
    return [(pages[i], c.pool.refs[pages[i]]) for i in range(lo // P, (hi + P - 1) // P) if c.pool.refs[pages[i]] > 1]


def test_snapshot_of_a_horizon_then_append_to_the_partial_page():
    """pages for 400 tokens, 150 committed, snapshot; the source appends 150..159.  Those positions live on page index 0 of the segment:
    copy-on-write must replace THAT page (not the horizon page behind it), and the snapshot must not see the source's values."""
    c = PagedCache(2, pool_pages=8, max_context=1024)
    c.ensure_tokens([400], NKV, HD, "cpu")
    _tags(c, 0, 0, 150, 1.0)
    c.lens = [150]
    s = c.snapshot()
    c.ensure_tokens([160], NKV, HD, "cpu")
    bad = _shared_pages_written(c, 0, 150, 160)
    assert not bad, f"the source writes positions 150..159 into (page, refs) {bad}, still shared with its snapshot"
    _tags(c, 0, 150, 160, 100.0)
    c.lens = [160]
    for l in range(2):
        got = s.packed_keys(l)[:, 0, 0]
        assert got.shape == (150,) and bool((got == 1.0 + l).all()), \
            f"layer {l}: the snapshot reads the source's append (page {s.pool.host_table[0][0]})"
        assert bool((c.packed_values(l)[:150, 0, 0] == 1.0 + l).all()) and bool((c.packed_values(l)[150:, 0, 0] == 100.0 + l).all())


def test_snapshot_at_a_page_edge_then_both_sides_append():
    """pages for 700 tokens, 256 committed, snapshot; BOTH sides append 256..299.  The page they write (index 1) was taken for the
    source's horizon: the snapshot must not share it, or the two appends land in one physical page."""
    c = PagedCache(2, pool_pages=8, max_context=1024)
    c.ensure_tokens([700], NKV, HD, "cpu")
    _tags(c, 0, 0, 256, 1.0)
    c.lens = [256]
    s = c.snapshot()
    for side, val in ((s, 300.0), (c, 200.0)):
        side.ensure_tokens([300], NKV, HD, "cpu")
        bad = _shared_pages_written(side, 0, 256, 300)
        assert not bad, f"an append to 256..299 writes (page, refs) {bad}, shared between the source and its snapshot"
        _tags(side, 0, 256, 300, val)
        side.lens = [300]
    for l in range(2):
        for side, val in ((c, 200.0), (s, 300.0)):
            k = side.packed_keys(l)[:, 0, 0]
            assert bool((k[:256] == 1.0 + l).all())
            assert bool((k[256:] == val + l).all()), \
                f"layer {l}: a side reads the other's append (page {side.pool.host_table[0][1]}, refs {side.pool.refs[side.pool.host_table[0][1]]})"


# --- model-based driver: random operation sequences against a dense shadow of every live cache

LAYERS, MAXC = 2, 1536          # 6 pages of reach per segment
TAG_FIELDS = 8                  # hd 8: K[pos] = (cache, segment, pos >> 8, pos & 255, write >> 8, write & 255, layer, 1 / 2 for K / V)


def _tag(cache_id, seg, lo, hi, write):
    pos = torch.arange(lo, hi)
    t = torch.empty(hi - lo, TAG_FIELDS)
    t[:, 0], t[:, 1], t[:, 2], t[:, 3] = cache_id, seg, pos // 256, pos % 256
    t[:, 4], t[:, 5] = write // 256, write % 256
    return t                     # (every field <= 255: exact in bf16)


def _explain(t):
    t = [int(v) for v in t.tolist()]
    return f"cache {t[0]} seg {t[1]} pos {t[2] * 256 + t[3]} write #{t[4] * 256 + t[5]}"


class _Model:
    def __init__(self, seed, nseg, pool_pages):
        self.rng = random.Random(seed)
        self.root = PagedCache(LAYERS, pool_pages=pool_pages, max_context=MAXC)
        self.root.ensure_tokens([0] * nseg, NKV, HD, "cpu")
        self.live = {0: self.root}                                    # cache id -> PagedCache (snapshots get ids 1, 2, ...)
        self.shadow = {0: [torch.zeros(MAXC, TAG_FIELDS) for _ in range(nseg)]}   # what each segment logically holds
        self.next_id, self.writes, self.log = 1, 0, []

    # -- state the invariants compare
    def _tables(self):
        return {cid: [list(p) for p in c.pool.host_table] for cid, c in self.live.items()}, \
               {cid: c.pool.table.clone() for cid, c in self.live.items()}

    def _state(self):
        return list(self.root.pool.refs), list(self.root.pool.free), *self._tables()

    def _write(self, cid, c, seg, lo, hi):
        """positions lo..hi-1 of segment `seg` (of `c`, a cache or a view of cache `cid`), through the host table, one write number"""
        self.writes += 1
        tag = _tag(cid, c._seg0 + seg, lo, hi, self.writes)
        pos = torch.arange(lo, hi)
        pg = torch.tensor(c.pool.host_table[c._seg0 + seg], dtype=torch.long)[pos // P]
        for l, sl in enumerate(c.slabs):
            for kv, val in ((0, 1.0), (1, 2.0)):
                t = tag.clone()
                t[:, 6], t[:, 7] = l, val
                if kv == 0:
                    sl.k[pg, 0, pos % P, :] = t.to(sl.k.dtype)
                else:
                    sl.vt[pg, 0, :, pos % P] = t.to(sl.vt.dtype)
        self.shadow[cid][c._seg0 + seg][lo:hi] = tag

    def _ensure(self, c, need):
        """ensure_tokens; a refused call must leave every table, the refs and the free list as they were"""
        before = self._state()
        try:
            c.ensure_tokens(need, NKV, HD, "cpu")
        except (RuntimeError, ValueError) as e:
            after = self._state()
            assert after[0] == before[0] and after[1] == before[1] and after[2] == before[2], f"refused request changed the pool: {e}"
            assert all(torch.equal(before[3][k], after[3][k]) for k in before[3]), f"refused request changed a device table: {e}"
            return False
        for s, n in enumerate(need):         # every page this call made writable is private
            if n > c.lens[s]:
                pages = c.pool.host_table[c._seg0 + s]
                for i in range(c.lens[s] // P, (n + P - 1) // P):
                    assert c.pool.refs[pages[i]] == 1, \
                        f"after ensure_tokens({need}) segment {s} (lens {c.lens[s]}) writes page {pages[i]} (index {i}), still shared: refs {c.pool.refs[pages[i]]}"
        return True

    # -- operations
    def step(self):
        r = self.rng
        cid = r.choice(sorted(self.live))
        c = self.live[cid]
        nseg = len(c.lens)
        seg = r.randrange(nseg)
        op = r.choices(["ensure", "write", "rewind", "snapshot", "view", "release", "exhaust", "drop"],
                       weights=[3, 6, 2, 2, 2, 1, 1, 0.5])[0]
        self.log.append((op, cid, seg, list(c.lens)))
        if op == "ensure":                   # a decode horizon past what is written
            need = [min(MAXC, n + r.randrange(0, 600)) if r.random() < 0.6 else n for n in c.lens]
            self._ensure(c, need)
        elif op == "write":                  # ensure + write q tokens at [lens, lens + q) (a prefill / decode chunk)
            q = r.choice([1, 2, r.randrange(1, 40), r.randrange(1, 300)])
            n = c.lens[seg]
            if n + q <= MAXC and self._ensure(c, [m + q if s == seg else m for s, m in enumerate(c.lens)]):
                self._write(cid, c, seg, n, n + q)
                c.lens[seg] = n + q
        elif op == "rewind":                 # gen_text puts the committed length back after an in-place decode
            c.lens[seg] = r.randrange(0, c.lens[seg] + 1)
        elif op == "snapshot":
            if len(self.live) < 5:
                s = c.snapshot()
                self.live[self.next_id] = s
                self.shadow[self.next_id] = [t.clone() for t in self.shadow[cid]]
                self.next_id += 1
        elif op == "view":                   # the serving pattern: prefill through a one-segment view, commit the length back
            v = c.view_segments(seg, seg + 1)
            n, q = v.lens[0], r.randrange(1, 300)
            if n + q <= MAXC and self._ensure(v, [n + q]):
                self._write(cid, v, 0, n, n + q)
                v.lens[0] = n + q
                c.lens[seg] = v.lens[0]
        elif op == "release":
            c.release(seg)
        elif op == "exhaust":                # more than the pool holds, or more than the table reaches
            need = [MAXC] * nseg if r.random() < 0.7 else [MAXC + r.randrange(1, 300)] + [0] * (nseg - 1)
            self._ensure(c, need)
        elif op == "drop" and cid != 0:      # a snapshot that is no longer needed gives its pages back
            for s in range(nseg):
                c.release(s)
            del self.live[cid], self.shadow[cid]

    # -- invariants
    def check(self):
        where = f"after {self.log[-1] if self.log else 'setup'} (ops: {self.log[-8:]})"
        pool = self.root.pool
        hosts = {}
        for cid, c in self.live.items():
            for s in range(len(c.lens)):
                pages = c.pool.host_table[s]
                hosts[id(pages)] = pages
                # 3. the device table row is the host table, padded with zeros
                row = c.pool.table[s]
                exp = torch.zeros_like(row)
                exp[:len(pages)] = torch.tensor(pages, dtype=row.dtype)
                assert torch.equal(row, exp), f"cache {cid} segment {s}: device row {row.tolist()} != host table {pages} {where}"
                assert 0 not in pages and len(set(pages)) == len(pages), f"cache {cid} segment {s} holds page 0 or a page twice: {pages} {where}"
                assert len(pages) * P >= c.lens[s], f"cache {cid} segment {s}: {len(pages)} pages for {c.lens[s]} tokens {where}"
            # 1. every layer / segment equals the shadow
            for l in range(LAYERS):
                for fn, kv in ((c.packed_keys, 1.0), (c.packed_values, 2.0)):
                    got = fn(l)
                    if got is None:
                        assert not any(c.lens)
                        continue
                    exp = torch.cat([self.shadow[cid][s][:n] for s, n in enumerate(c.lens)], 0)
                    exp[:, 6], exp[:, 7] = l, kv
                    got = got[:, 0].float()
                    if not torch.equal(got, exp):
                        r = int((got != exp).any(1).nonzero()[0])
                        s = next(i for i in range(len(c.lens)) if r < sum(c.lens[:i + 1]))
                        pos = r - sum(c.lens[:s])
                        pg = c.pool.host_table[s][pos // P]
                        raise AssertionError(f"cache {cid} segment {s} position {pos} (page {pg}, refs {pool.refs[pg]}) layer {l} "
                                             f"{'K' if kv == 1 else 'V'}: holds {_explain(got[r])}, expected {_explain(exp[r])} {where}")
        # 2. reference counts = distinct host tables holding the page; the free list is exactly the unreferenced pages
        count = [0] * pool.npages
        for pages in hosts.values():
            for p in set(pages):
                count[p] += 1
        assert count == pool.refs, f"refs {[(p, r, n) for p, (r, n) in enumerate(zip(pool.refs, count)) if r != n]} (page, refs, tables) {where}"
        assert len(set(pool.free)) == len(pool.free), f"free list has duplicates {where}"
        assert set(pool.free) == {p for p in range(1, pool.npages) if pool.refs[p] == 0}, f"free list != unreferenced pages {where}"


@pytest.mark.parametrize("block", range(8))
def test_paged_cache_against_a_dense_shadow(block):
    """320 seeds x 60 random operations on a 3-segment cache over a 20-page pool (snapshots of snapshots, horizons, rewinds, views,
    releases, refused requests); every invariant after every operation"""
    for seed in range(block * 40, block * 40 + 40):
        rng = random.Random(10_000 + seed)
        m = _Model(seed, nseg=rng.choice([1, 2, 3]), pool_pages=rng.choice([12, 20, 28]))
        m.check()
        for _ in range(60):
            m.step()
            m.check()
