"""Host side of prefix sharing in the paged batcher (serving.ContinuousBatcher(share_prefixes=True)): chunk keys, the partition of an
admission group into hits, leaders and followers, and the least-recently-used table of retained prefixes.  Pure host code - no GPU.

A request's chunks are its images in order, then its prompt: the batcher's prefill order.  The prefix key after chunk i is the tuple of
the chunk keys 0..i.  Sharing happens at chunk boundaries only, where it is exact: a row's bits do not depend on what else is in the
batch, so the KV of "images 0..j" is the same whichever request computed it - as long as the pass that computed
it ran in the same GEMM family (up to 64 rows / above) as the pass the request would have run itself.
"""
import hashlib
from collections import OrderedDict

import torch


def image_key(image):
    """16-byte blake2b digest of the raw input: a tensor's dtype, shape and the bytes of a contiguous CPU copy; a PIL image's mode, size
    and tobytes().  (The transform is not part of the key: a batcher has one.)"""
    h = hashlib.blake2b(digest_size=16)
    if isinstance(image, torch.Tensor):
        t = image.detach().cpu().contiguous()
        h.update(repr(("tensor", str(t.dtype), tuple(t.shape))).encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    elif hasattr(image, "tobytes") and hasattr(image, "mode") and hasattr(image, "size"):
        h.update(repr(("pil", image.mode, tuple(image.size))).encode())
        h.update(image.tobytes())
    else:
        raise TypeError(f"no prefix key for an image of type {type(image).__name__}: pass submit(image_keys=[...])")
    return h.digest()


def chunk_keys(images, prompt_ids, image_keys=None):
    """The chunk keys of one request: ("img", key) per image - the caller's own hashable keys where given, else image_key - then
    ("txt", the packed token ids of the prompt, wrapper included)."""
    if image_keys is not None and len(image_keys) != len(images):
        raise ValueError(f"image_keys: {len(image_keys)} keys for {len(images)} images")
    keys = image_keys if image_keys is not None else [image_key(im) for im in images]
    return tuple(("img", k) for k in keys) + (("txt", tuple(int(t) for t in prompt_ids)),)


def plan_group(chains, cached):
    """The hit / leader / follower partition of an admission group - a pure function.  chains[r]: request r's chunk keys;
    cached(prefix key) -> bool.  Returns (states, leader): states[r][j] is
      "hit"     chunk j lies inside the longest cached chain of request r (the deepest i with chains[r][:i + 1] cached: the request
                adopts ONCE, there, not chunk by chunk),
      "lead"    r is the first request of the group whose prefix key after chunk j is new: it computes chunk j,
      "follow"  an earlier request of the group leads the same prefix key: leader[r][j] is that request (None otherwise).
    A request's states always read hit* follow* lead*: a leader's later prefixes extend a key nobody else had first."""
    depth = []
    for c in chains:
        d = -1
        for i in range(len(c)):
            if cached(c[:i + 1]):
                d = i
        depth.append(d)
    states = [[None] * len(c) for c in chains]
    leader = [[None] * len(c) for c in chains]
    for j in range(max([len(c) for c in chains] + [0])):
        first = {}
        for r, c in enumerate(chains):
            if j >= len(c):
                continue
            if j <= depth[r]:
                states[r][j] = "hit"
            elif c[:j + 1] in first:
                states[r][j], leader[r][j] = "follow", first[c[:j + 1]]
            else:
                first[c[:j + 1]] = r
                states[r][j] = "lead"
    return states, leader


def adopt_point(states):
    """Of one request's states: the index of its last chunk that is not led (-1: it leads everything) - where it adopts."""
    return max([j for j, s in enumerate(states) if s != "lead"] + [-1])


class PrefixTable:
    """Retained prefixes by prefix key, least recently used first.  An entry is (handle, rope position after the chunk); the pages the
    entries hold are counted as DISTINCT pages, tails included (the entries of one chain share their full pages)."""

    def __init__(self, cache, max_pages, stats=None):
        self.cache, self.max_pages = cache, int(max_pages)
        self.entries = OrderedDict()
        self.stats = {} if stats is None else stats        # "prefix_evictions" is counted here (the batcher passes its own dict)
        self.stats.setdefault("prefix_evictions", 0)

    def __contains__(self, key):
        return key in self.entries

    def __len__(self):
        return len(self.entries)

    def get(self, key):
        """the entry of `key`; it and the inner nodes of its chain become the most recently used"""
        for i in range(1, len(key) + 1):
            if key[:i] in self.entries:
                self.entries.move_to_end(key[:i])
        return self.entries[key]

    def put(self, key, handle, rope):
        self.entries[key] = (handle, rope)

    def pages_held(self):
        return len({p for h, _ in self.entries.values() for p in h.pages})

    def evict_one(self, keep=()):
        """drop the least recently used entry that is not in `keep`; False when there is none"""
        for key in self.entries:
            if key not in keep:
                self.cache.drop_prefix(self.entries.pop(key)[0])
                self.stats["prefix_evictions"] += 1
                return True
        return False

    def trim(self):
        """hold the bound: least recently used entries go first"""
        while self.entries and self.pages_held() > self.max_pages:
            self.evict_one()

    def make_room(self, want, keep=()):
        """evict least recently used entries until `want` pages are free or nothing is left to evict; the caller's page-taking call
        then fits, or fails exactly as it would without this table"""
        while want > len(self.cache.pool.free) and self.evict_one(keep):
            pass

    def clear(self):
        for h, _ in self.entries.values():
            self.cache.drop_prefix(h)
        self.entries.clear()
