"""KV cache as in-place slabs.

Drop-in for the reference's ``NaiveCache`` (codes/modeling/unimedvl/qwen2_navit.py:207-221):
same constructor ``NaiveCache(num_layers)``, ``num_layers`` / ``seq_lens`` properties,
and it survives ``copy.deepcopy`` (the inferencer snapshots contexts that way,
codes/inferencer.py:587,600,607,261).  The reference re-allocates and re-scatters the
whole ``[sum K, kvh, hd]`` tensor on every forward (qwen2_navit.py:585-600); here each
layer owns  K [seg][kvh][cap][hd]  and  V^T [seg][kvh][hd][cap]  bf16 slabs that are
appended in place, with the per-sample lengths kept on the host.
"""
import torch

from . import ops


def _round_up(x, m):
    return (x + m - 1) // m * m


class NaiveCache:
    def __init__(self, num_layers):
        self._num_layers = num_layers
        self.slabs = None          # list[KVSlab] once materialised
        self.lens = []             # committed tokens per segment (host ints)
        self.nkv = self.hd = None
        self.device = None
        self._borrowed = False     # slabs belong to another cache (snapshot()): copy before the first write
        self.reserved = False      # reserve() was called: slab addresses are stable for the life of the cache

    # --- prefix sharing ("prefix-sharing of the three CFG contexts instead of deepcopy")
    def snapshot(self):
        """O(1) logical copy: shares this cache's slabs and freezes the current lengths.  Safe because tokens are only ever
        APPENDED in place beyond `lens` (this cache may go on appending or decoding; the snapshot never sees those slots)
        and because a snapshot copies itself before ITS first write (copy-on-write in ensure()).  Replaces the whole-KV
        ``deepcopy(gen_context)`` the reference takes per text item (inferencer.py:261,587,600,607)."""
        c = NaiveCache(self._num_layers)
        c.lens = list(self.lens)
        c.nkv, c.hd, c.device = self.nkv, self.hd, self.device
        c.slabs = self.slabs
        c._borrowed = self.slabs is not None
        return c

    def shares_storage_with(self, other):
        """True when both caches read the same slab memory (one is a snapshot of the other, or both of a third)."""
        if self.slabs is None or other.slabs is None or len(self.slabs) != len(other.slabs):
            return False
        return all(a.k.data_ptr() == b.k.data_ptr() and a.vt.data_ptr() == b.vt.data_ptr() and a.cap == b.cap
                   for a, b in zip(self.slabs, other.slabs))

    def _materialize(self, need_cap):
        """private copy of the visible prefix (what deepcopy would have made when the snapshot was taken)"""
        nseg = len(self.lens)
        cap = _round_up(max(need_cap, self.slabs[0].cap if self.slabs else 0, 256), 256)
        keep = _round_up(max(max(self.lens), 1), 32)
        new = []
        for old in self.slabs:
            s = ops.KVSlab(nseg, self.nkv, cap, self.hd, self.device)
            s.k[:, :, :keep].copy_(old.k[:, :, :keep])
            s.vt[:, :, :, :keep].copy_(old.vt[:, :, :, :keep])
            new.append(s)
        self.slabs = new
        self._borrowed = False

    # --- reference-compatible surface
    @property
    def num_layers(self):
        return self._num_layers

    @property
    def seq_lens(self):
        return sum(self.lens)

    @property
    def key_cache(self):
        """{layer: [sum K, kvh, hd]} view materialised on demand (tests / debugging)."""
        return {l: self.packed_keys(l) for l in range(self._num_layers)}

    @property
    def value_cache(self):
        return {l: self.packed_values(l) for l in range(self._num_layers)}

    def packed_keys(self, layer):
        if self.slabs is None or not any(self.lens):
            return None
        return torch.cat([self.slabs[layer].k[s, :, :n].transpose(0, 1) for s, n in enumerate(self.lens)], 0)

    def packed_values(self, layer):
        if self.slabs is None or not any(self.lens):
            return None
        return torch.cat([self.slabs[layer].vt[s, :, :, :n].permute(2, 0, 1) for s, n in enumerate(self.lens)], 0)

    # --- slab management
    @property
    def cap(self):
        return 0 if self.slabs is None else self.slabs[0].cap

    def ensure(self, nseg, need_cap, nkv, hd, device):
        """Make room for `need_cap` tokens per segment (committed + the call's new tokens)."""
        need_cap = _round_up(max(need_cap, 32), 32)
        if self.slabs is None:
            cap = _round_up(max(need_cap, 256), 256)
            self.slabs = [ops.KVSlab(nseg, nkv, cap, hd, device) for _ in range(self._num_layers)]
            self.lens = [0] * nseg
            self.nkv, self.hd, self.device = nkv, hd, device
            return
        if nseg != len(self.lens):
            raise ValueError(f"cache holds {len(self.lens)} samples, call has {nseg}")
        if self._borrowed:          # every forward / decode calls ensure() before it writes: copy-on-write happens here
            self._materialize(need_cap)
        if need_cap > self.cap:
            cap = _round_up(max(need_cap, 2 * self.cap), 256)
            keep = max(self.lens)
            new = []
            for old in self.slabs:
                s = ops.KVSlab(nseg, self.nkv, cap, self.hd, self.device)
                if keep:
                    s.k[:, :, :keep].copy_(old.k[:, :, :keep])
                    s.vt[:, :, :, :keep].copy_(old.vt[:, :, :, :keep])
                new.append(s)
            self.slabs = new

    def reserve(self, nseg, cap, nkv, hd, device):
        """Pre-size (bench / serving) so that decode never re-allocates.  A reserved cache keeps its slab addresses, which is
        what lets fixed-shape prefills into it replay from a HIP graph (bagel.Bagel.forward_cache_update_vit)."""
        self.ensure(nseg, cap, nkv, hd, device)
        self.reserved = True

    @staticmethod
    def merged(caches, nsegs, extra, nkv, hd, device):
        """One cache whose segments are the segments of `caches` back to back (contexts that hold
        different tokens for the same samples, e.g. the three CFG contexts of bagel.py:1120-1171),
        with room for `extra` more tokens per segment.  Lets independent passes run as ONE packed
        forward.  `nsegs[i]` = samples in caches[i] (needed for caches that are still empty)."""
        lens = []
        for c, n in zip(caches, nsegs):
            lens += list(c.lens) if c.slabs is not None else [0] * n
        m = NaiveCache(caches[0].num_layers)
        m.ensure(len(lens), max(lens) + extra, nkv, hd, device)
        m.lens = lens
        base = 0
        for c, n in zip(caches, nsegs):
            if c.slabs is not None and max(c.lens) > 0:
                keep = _round_up(max(c.lens), 32)
                for dst, src in zip(m.slabs, c.slabs):
                    dst.k[base:base + n, :, :keep].copy_(src.k[:, :, :keep])
                    dst.vt[base:base + n, :, :, :keep].copy_(src.vt[:, :, :, :keep])
            base += n
        return m

    def view_segments(self, start, end):
        """A cache over segments [start, end) sharing this cache's memory (no copy)."""
        if self._borrowed:
            self._materialize(self.cap)
        v = NaiveCache(self._num_layers)
        v.lens = list(self.lens[start:end])
        v.nkv, v.hd, v.device = self.nkv, self.hd, self.device
        v.slabs = [ops.KVSlab.from_tensors(s.k[start:end], s.vt[start:end]) for s in self.slabs]
        return v

    def __deepcopy__(self, memo):
        c = NaiveCache(self._num_layers)
        c.lens = list(self.lens)
        c.nkv, c.hd, c.device = self.nkv, self.hd, self.device
        if self.slabs is not None:
            keep = _round_up(max(max(self.lens), 1), 32)
            cap = self.cap
            c.slabs = []
            for old in self.slabs:
                s = ops.KVSlab(len(self.lens), self.nkv, cap, self.hd, self.device)
                s.k[:, :, :keep].copy_(old.k[:, :, :keep])
                s.vt[:, :, :, :keep].copy_(old.vt[:, :, :, :keep])
                c.slabs.append(s)
        return c


class _PagePool:
    """Allocator state shared by a PagedCache and its views / snapshots: the per-layer pools, the free list, page reference counts."""

    def __init__(self, num_layers, npages, nkv, hd, device, nseg, max_pages):
        if npages * nkv * ops.KV_PAGE * hd * 2 > 2 ** 31 - 1:       # the LDS-shared prefill kernels reach a page through a 32-bit byte offset
            raise ValueError(f"paged KV pool of {npages} pages x {nkv * ops.KV_PAGE * hd * 2} bytes exceeds 2 GiB per layer and operand")
        self.table = torch.zeros((nseg, max_pages), dtype=torch.int32, device=device)      # entry p of segment s: pool page of keys p*256..
        self.host_table = [[] for _ in range(nseg)]                                       # pages each segment owns, in order
        self.slabs = [ops.PagedSlab(npages, nkv, hd, device, self.table) for _ in range(num_layers)]
        self.free = list(range(npages - 1, 0, -1))       # page 0 stays unused: a table entry of 0 is "no page" (reads of it are masked anyway)
        self.refs = [0] * npages
        self.npages, self.nkv, self.hd, self.device = npages, nkv, hd, device

    def alloc(self):
        if not self.free:
            raise RuntimeError(f"paged KV pool exhausted ({self.npages - 1} pages of {ops.KV_PAGE} tokens): raise pool_pages")
        p = self.free.pop()
        self.refs[p] = 1
        return p

    def unref(self, p):
        self.refs[p] -= 1
        if self.refs[p] == 0:
            self.free.append(p)


class PrefixHandle:
    """A context prefix of n tokens in a page pool (PagedCache.retain_prefix): its n // 256 full pages, shared by reference count, and -
    n % 256 != 0 - the page that holds its tail.  owned: the handle holds those references and that page (False: live_prefix)."""
    __slots__ = ("n", "full", "tail", "owned")

    def __init__(self, n, full, tail, owned):
        self.n, self.full, self.tail, self.owned = n, list(full), tail, owned

    @property
    def pages(self):
        return self.full + ([self.tail] if self.tail is not None else [])


class PagedCache:
    """Block-table KV cache: every layer owns ONE pool of 256-token pages, K [page][kvh][256][hd] and
    V^T [page][kvh][hd][256], that all segments draw from; a segment's context is the list of its pages (`table` on the device).
    A context grows by taking pages - nothing is copied or re-allocated, the pool is shared by short and long requests - and a finished
    request returns its pages (`release`).  snapshot() shares the pages of the prefix (reference counts); a page either side is about to
    write while the other still holds it is replaced by a private one first (copy-on-write in ensure_tokens).

    Same surface as NaiveCache for the paths that take it: LanguageModel.forward_inference (prefill: umv_qkv_post writes through the
    table, the attention of a paged call runs on the per-wave kernel), decode.DecodeSession (the captured step reads the table from
    device memory: pages for the whole decode horizon are taken before the capture) and serving.ContinuousBatcher(paged=True).  The
    reference's NaiveCache is unbounded because it re-merges the cache on every forward (qwen2_navit.py:585-600)."""

    def __init__(self, num_layers, pool_pages=1024, max_context=32768):
        self._num_layers = num_layers
        self.pool_pages, self.max_pages = int(pool_pages), (int(max_context) + ops.KV_PAGE - 1) // ops.KV_PAGE
        self.pool = None
        self.lens = []
        self._seg0 = 0                      # view_segments(): first segment of the pool's table this cache covers
        self.nkv = self.hd = self.device = None
        self.reserved = False               # (no HIP-graph prefills into a paged cache: the table changes between calls)

    # --- NaiveCache-compatible surface
    @property
    def num_layers(self):
        return self._num_layers

    @property
    def seq_lens(self):
        return sum(self.lens)

    @property
    def cap(self):
        return self.max_pages * ops.KV_PAGE

    @property
    def slabs(self):
        if self.pool is None:
            return None
        if self._seg0 == 0 and len(self.lens) == self.pool.table.shape[0]:
            return self.pool.slabs
        # a view: the same pools behind a slice of the table rows
        t = self.pool.table[self._seg0:self._seg0 + len(self.lens)]
        out = []
        for s in self.pool.slabs:
            v = ops.PagedSlab.__new__(ops.PagedSlab)
            v.k, v.vt, v.table, v.nkv, v.hd, v.cap = s.k, s.vt, t, s.nkv, s.hd, s.cap
            out.append(v)
        return out

    def _pages(self, seg):
        return self.pool.host_table[self._seg0 + seg]

    def ensure(self, nseg, need_cap, nkv, hd, device):
        """NaiveCache.ensure's contract: room for need_cap tokens in EVERY segment (callers that know per-segment needs use ensure_tokens)"""
        self.ensure_tokens([need_cap] * nseg, nkv, hd, device)

    def ensure_tokens(self, need, nkv, hd, device):
        """Pages for need[s] tokens in segment s (committed + the call's new tokens); only segments that grow take pages.  Every page
        this call makes writable - page indices lens[s] // 256 .. ceil(need[s] / 256) - 1 - is private to this cache afterwards: one
        still shared with a snapshot (refs > 1) is replaced by a fresh page (copy-on-write; only the partially filled page at lens[s]
        carries data over, the others hold nothing committed yet).  All or nothing: a refused call takes and changes no page."""
        nseg = len(need)
        if self.pool is None:
            self.pool = _PagePool(self._num_layers, self.pool_pages, nkv, hd, device, nseg, self.max_pages)
            self.lens = [0] * nseg
            self.nkv, self.hd, self.device = nkv, hd, device
        if nseg != len(self.lens):
            raise ValueError(f"cache holds {len(self.lens)} samples, call has {nseg}")
        P = ops.KV_PAGE
        want = self.pages_wanted(need)        # all-or-nothing: check the reach and the pool before taking a single page
        if want > len(self.pool.free):
            raise RuntimeError(f"paged KV pool exhausted: {want} pages wanted, {len(self.pool.free)} of {self.pool.npages - 1} free "
                               f"({P} tokens each): raise pool_pages")
        changed = []
        for s, n in enumerate(need):
            pages = self._pages(s)
            if n > self.lens[s]:
                # copy-on-write: a page this call writes is shared with a snapshot (or the snapshot's source)
                for i in range(self.lens[s] // P, min(len(pages), (n + P - 1) // P)):
                    old = pages[i]
                    if self.pool.refs[old] == 1:
                        continue
                    new = self.pool.alloc()
                    if i * P < self.lens[s]:         # the partially filled page: its committed head is this cache's context
                        for sl in self.pool.slabs:
                            sl.k[new].copy_(sl.k[old])
                            sl.vt[new].copy_(sl.vt[old])
                    self.pool.unref(old)
                    pages[i] = new
                    changed.append((s, i, new))
            while len(pages) * P < n:
                pages.append(self.pool.alloc())
                changed.append((s, len(pages) - 1, pages[-1]))
        if changed:
            idx = torch.tensor([[self._seg0 + s, p] for s, p, _ in changed], dtype=torch.long)
            val = torch.tensor([v for _, _, v in changed], dtype=torch.int32)
            self.pool.table.index_put_((idx[:, 0].to(self.device), idx[:, 1].to(self.device)), val.to(self.device))

    def pages_wanted(self, need):
        """Pure query: the pages ensure_tokens(need) would take from the free list - the pages each segment lacks for need[s] tokens
        plus one per shared page the call would write (copy-on-write).  ValueError beyond the page table's reach, as ensure_tokens."""
        P = ops.KV_PAGE
        want = 0
        for s, n in enumerate(need):
            if n > self.cap:
                raise ValueError(f"segment {s}: {n} tokens exceed the page table's reach of {self.cap} (max_context)")
            if self.pool is None:
                want += (n + P - 1) // P
                continue
            pages = self._pages(s)
            want += max(0, (n + P - 1) // P - len(pages))
            if n > self.lens[s]:
                want += sum(self.pool.refs[p] > 1 for p in pages[self.lens[s] // P:(n + P - 1) // P])
        return want

    def reserve(self, nseg, cap, nkv, hd, device):
        """NaiveCache.reserve pre-sizes slabs; here it only creates the pool and the table (pages are taken as contexts grow)"""
        self.ensure_tokens([0] * nseg, nkv, hd, device)

    def release(self, seg):
        """Return segment `seg`'s pages to the pool (its request is finished), reset its length and zero its row of the device table:
        a stray write through the released row lands in page 0, which is never handed out, not in a page another request owns now."""
        for p in self._pages(seg):
            self.pool.unref(p)
        self._pages(seg).clear()
        self.pool.table[self._seg0 + seg].zero_()
        self.lens[seg] = 0

    def pages_in_use(self):
        return self.pool.npages - 1 - len(self.pool.free)

    # --- prefixes shared at page granularity (serving.ContinuousBatcher(share_prefixes=True))
    # A partially filled page is never shared: every holder of a prefix - a retained handle, and each segment that adopts one - refers
    # to the prefix's FULL pages (reference counts) and owns a private copy of the first n % 256 tokens of the partial page.  So no
    # holder ever writes a shared page (its write position, n, lies in its own tail), and ensure_tokens' copy-on-write has nothing to do.
    def live_prefix(self, seg):
        """A handle on segment `seg`'s context as it stands: it owns nothing (no reference, no page), so it is good for an adopt_prefix
        that is queued before the segment is written or released again, and for nothing else; drop_prefix ignores it."""
        P, n = ops.KV_PAGE, self.lens[seg]
        pages = self._pages(seg)
        return PrefixHandle(n, list(pages[:n // P]), pages[n // P] if n % P else None, False)

    def retain_prefix(self, segs):
        """Keep the context of a segment (an index -> one handle) or of several (a list -> a list of handles): a reference to each of
        its lens[seg] // 256 full pages and, with lens[seg] % 256 != 0, one new page holding a copy of the tail.  All the tail copies of
        the call are one launch.  All or nothing: a refused call (RuntimeError: pool exhausted) takes no page and no reference."""
        one = not isinstance(segs, (list, tuple))
        live = [self.live_prefix(s) for s in ([segs] if one else segs)]
        self._want_free(sum(h.tail is not None for h in live), "retain_prefix")
        out, copies = [], []
        for h in live:
            for p in h.full:
                self.pool.refs[p] += 1
            tail = None
            if h.tail is not None:
                tail = self.pool.alloc()
                copies.append((h.tail, tail, h.n % ops.KV_PAGE))
            out.append(PrefixHandle(h.n, h.full, tail, True))
        self._copy_tails(copies)
        return out[0] if one else out

    def adopt_prefix(self, seg, handle=None):
        """adopt_prefix(seg, handle) or adopt_prefix([(seg, handle), ...]): every segment, which must hold nothing (a released one is
        fine), becomes a holder of its handle's prefix - a reference to each full page, a private page with a copy of the handle's tail,
        its table row written and lens[seg] set.  One launch for all the tail copies.  All or nothing against the free list."""
        pairs = [(seg, handle)] if handle is not None else list(seg)
        if len({s for s, _ in pairs}) != len(pairs):
            raise ValueError("adopt_prefix: a segment is named twice")
        for s, h in pairs:
            if self.lens[s] or self._pages(s):
                raise ValueError(f"adopt_prefix: segment {s} holds {self.lens[s]} tokens / {len(self._pages(s))} pages; release it first")
            if h.n > self.cap:
                raise ValueError(f"segment {s}: {h.n} tokens exceed the page table's reach of {self.cap} (max_context)")
        self._want_free(sum(h.tail is not None for _, h in pairs), "adopt_prefix")
        copies = []
        for s, h in pairs:
            pages = self._pages(s)
            for p in h.full:
                self.pool.refs[p] += 1
                pages.append(p)
            if h.tail is not None:
                pages.append(self.pool.alloc())
                copies.append((h.tail, pages[-1], h.n % ops.KV_PAGE))
            if pages:
                self.pool.table[self._seg0 + s, :len(pages)] = torch.tensor(pages, dtype=torch.int32).to(self.pool.table.device)
            self.lens[s] = h.n
        self._copy_tails(copies)

    def drop_prefix(self, handle):
        """Give a retained handle's pages back: one reference of each full page and the tail page, each exactly once (a second drop
        of the same handle, or a drop of a live_prefix handle, does nothing)."""
        if not handle.owned:
            return
        for p in handle.full:
            self.pool.unref(p)
        if handle.tail is not None:
            self.pool.unref(handle.tail)
        handle.owned = False

    def _want_free(self, want, what):
        if want > len(self.pool.free):
            raise RuntimeError(f"paged KV pool exhausted: {what} wants {want} pages, {len(self.pool.free)} of {self.pool.npages - 1} free "
                               f"({ops.KV_PAGE} tokens each): raise pool_pages")

    def _copy_tails(self, copies):
        """(source page, destination page, tokens) in every layer, K and V^T: tokens rounded up to 8 (the copy's 16-byte unit; what lies
        behind a holder's length is never read).  A pool on the GPU: ONE umv_beam_kv_copy launch; a CPU pool: the same range by slices."""
        if not copies:
            return
        rows = [(src, dst, _round_up(t, 8), 0) for src, dst, t in copies]
        slabs = self.pool.slabs
        if slabs[0].k.is_cuda:
            if getattr(self.pool, "prefix_pools", None) is None:
                self.pool.prefix_pools = ops.beam_pool_pointers(slabs)
            ops.beam_kv_copy(torch.tensor(rows, dtype=torch.int32).to(slabs[0].k.device), self.pool.prefix_pools, slabs)
            return
        for src, dst, t, _ in rows:
            for sl in slabs:
                sl.k[dst, :, :t] = sl.k[src, :, :t]
                sl.vt[dst, :, :, :t] = sl.vt[src, :, :, :t]

    def snapshot(self):
        """Logical copy sharing the pages of the current contexts (reference counted): the first ceil(lens[s] / 256) pages of each
        segment.  Pages past that (a decode horizon taken before a rewind of `lens`) stay with this cache alone.  Appends by either side
        are isolated: ensure_tokens replaces every shared page the append will write (copy-on-write).  The snapshot has a table of its
        own over the same pools and allocator; release() its segments to give its pages back."""
        c = PagedCache(self._num_layers, self.pool_pages, self.max_pages * ops.KV_PAGE)
        c.lens = list(self.lens)
        c.nkv, c.hd, c.device = self.nkv, self.hd, self.device
        if self.pool is not None:
            c.pool = self._over_same_pools(len(self.lens)).pool
            c.pool.host_table = [list(self._pages(s)[:(n + ops.KV_PAGE - 1) // ops.KV_PAGE]) for s, n in enumerate(self.lens)]
            rows = torch.zeros(c.pool.table.shape, dtype=torch.int32)
            for s, pages in enumerate(c.pool.host_table):
                rows[s, :len(pages)] = torch.tensor(pages, dtype=torch.int32)
            c.pool.table.copy_(rows)
            for pages in c.pool.host_table:
                for p in pages:
                    self.pool.refs[p] += 1
        return c

    def _over_same_pools(self, nrows):
        """An empty cache with a table of `nrows` rows of its own over this cache's pools and allocator (snapshot(), fork_beams())."""
        src = self.pool
        c = PagedCache(self._num_layers, self.pool_pages, self.max_pages * ops.KV_PAGE)
        c.nkv, c.hd, c.device = self.nkv, self.hd, self.device
        c.pool = _PagePool.__new__(_PagePool)
        c.pool.host_table = [[] for _ in range(nrows)]
        c.pool.table = torch.zeros((nrows, src.table.shape[1]), dtype=torch.int32, device=src.table.device)
        c.pool.free, c.pool.refs = src.free, src.refs            # ONE allocator: shared lists
        c.pool.npages, c.pool.nkv, c.pool.hd, c.pool.device = src.npages, src.nkv, src.hd, src.device
        c.pool.slabs = []
        for sl in src.slabs:
            v = ops.PagedSlab.__new__(ops.PagedSlab)
            v.k, v.vt, v.table, v.nkv, v.hd, v.cap = sl.k, sl.vt, c.pool.table, sl.nkv, sl.hd, sl.cap
            c.pool.slabs.append(v)
        return c

    def fork_beams(self, K, horizon):
        """The KV plan of beam search decode (include/unimedvl_hip.h, beam search decode; beam.BeamDecodeSession): a throwaway cache
        over the same pools and allocator with K table rows per segment, row b * K + i for beam i of segment b.  Every row shares
        segment b's FULL prompt pages (reference counts) and owns, for every page index from j0 = lens[b] // 256 up to the one slot
        lens[b] + horizon - 1 falls in, TWO private pages: a current one, which its table row names, and a spare.  The partially
        filled prompt page is copied into every row's current page at j0.  beam_own (int32 [rows, NP, 2] on the device: the pair of
        row r and page index j0 + q) and beam_j0 (int32 [segments]) are what the step end reads.  The device rewrites the table rows
        while it decodes; nothing is ever read back: release_all() returns every page by the host lists, each exactly once.
        All or nothing: a refused fork (RuntimeError: pool exhausted; ValueError: past the table's reach) takes no page."""
        if self.pool is None:
            raise ValueError("fork_beams: the cache holds no context")
        if isinstance(K, bool) or int(K) != K or K < 1 or horizon < 1:
            raise ValueError(f"fork_beams: K (got {K!r}) and horizon (got {horizon!r}) must be positive integers")
        P, K = ops.KV_PAGE, int(K)
        B = len(self.lens)
        j0 = [n // P for n in self.lens]
        npg = [(n + horizon - 1) // P - j + 1 for n, j in zip(self.lens, j0)]
        if max(j + m for j, m in zip(j0, npg)) > self.max_pages:
            raise ValueError(f"fork_beams: {max(self.lens) + horizon} tokens exceed the page table's reach of {self.cap} (max_context)")
        want = 2 * K * sum(npg)
        if want > len(self.pool.free):
            raise RuntimeError(f"paged KV pool exhausted: {want} pages wanted, {len(self.pool.free)} of {self.pool.npages - 1} free "
                               f"({P} tokens each): raise pool_pages")
        c = self._over_same_pools(B * K)
        c.lens = [n for n in self.lens for _ in range(K)]
        NP = max(npg)
        rows = torch.zeros(c.pool.table.shape, dtype=torch.int32)
        own = torch.zeros((B * K, NP, 2), dtype=torch.int32)
        c.beam_spares = [[] for _ in range(B * K)]
        for b in range(B):
            shared = list(self._pages(b)[:j0[b]])
            for r in range(b * K, (b + 1) * K):
                for p in shared:
                    self.pool.refs[p] += 1
                cur = [self.pool.alloc() for _ in range(npg[b])]
                c.beam_spares[r] = [self.pool.alloc() for _ in range(npg[b])]
                c.pool.host_table[r] = shared + cur
                rows[r, :len(shared) + len(cur)] = torch.tensor(shared + cur, dtype=torch.int32)
                own[r, :npg[b], 0] = torch.tensor(cur, dtype=torch.int32)
                own[r, :npg[b], 1] = torch.tensor(c.beam_spares[r], dtype=torch.int32)
            if self.lens[b] % P:                     # the partially filled prompt page: every row's current page at j0 starts as a copy
                at = own[b * K:(b + 1) * K, 0, 0].to(device=self.device, dtype=torch.int64)
                old = self._pages(b)[j0[b]]
                for sl in self.pool.slabs:
                    sl.k[at] = sl.k[old].clone()
                    sl.vt[at] = sl.vt[old].clone()
        c.pool.table.copy_(rows)
        c.beam_own = own.to(self.device)
        c.beam_j0 = torch.tensor(j0, dtype=torch.int32).to(self.device)
        c.beam_K = K
        return c

    def release_all(self):
        """Return every page this cache holds to the pool by the host lists - a fork's spares included -, each exactly once, and
        zero the device table."""
        for seg in range(len(self.lens)):
            for p in self._pages(seg) + (self.beam_spares[seg] if getattr(self, "beam_spares", None) else []):
                self.pool.unref(p)
            self._pages(seg).clear()
            if getattr(self, "beam_spares", None):
                self.beam_spares[seg] = []
            self.lens[seg] = 0
        self.pool.table[self._seg0:self._seg0 + len(self.lens)].zero_()

    def view_segments(self, start, end):
        """A cache over segments [start, end) of the same table and pools (no copy)."""
        v = PagedCache(self._num_layers, self.pool_pages, self.max_pages * ops.KV_PAGE)
        v.pool, v._seg0 = self.pool, self._seg0 + start
        v.lens = list(self.lens[start:end])
        v.nkv, v.hd, v.device = self.nkv, self.hd, self.device
        return v

    def packed_keys(self, layer):
        if self.pool is None or not any(self.lens):
            return None
        sl = self.pool.slabs[layer]
        out = []
        for s, n in enumerate(self.lens):
            pg = self._pages(s)
            for i in range((n + ops.KV_PAGE - 1) // ops.KV_PAGE):
                m = min(ops.KV_PAGE, n - i * ops.KV_PAGE)
                out.append(sl.k[pg[i], :, :m].transpose(0, 1))
        return torch.cat(out, 0)

    def packed_values(self, layer):
        if self.pool is None or not any(self.lens):
            return None
        sl = self.pool.slabs[layer]
        out = []
        for s, n in enumerate(self.lens):
            pg = self._pages(s)
            for i in range((n + ops.KV_PAGE - 1) // ops.KV_PAGE):
                m = min(ops.KV_PAGE, n - i * ops.KV_PAGE)
                out.append(sl.vt[pg[i], :, :, :m].permute(2, 0, 1))
        return torch.cat(out, 0)
