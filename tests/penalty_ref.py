"""numpy restatement of the logit penalties (include/unimedvl_hip.h, "logit penalties and bias") for the tests.

    a = l[n]                                                      l = float32(stored bf16 logit)
    if seen(n) and r != 1:  a = a * r if a < 0 else a / r         seen = generated before or in the context set
    if c[n] > 0:            a = a - (presence + frequency * float32(c[n]))
    if bias[n] != 0:        a = a + bias[n]
    l'[n] = bf16_round_nearest_even(a)

Every operation is one float32 numpy operation, so one rounding each; bf16 rounding is done on the bit pattern.  A History is the
host-side picture of what the kernel keeps per row: the count words, the visit list (static entries first: the context columns in order
of first appearance, then the biased columns that are not in the context), its length (-1 = fresh) and the bias of the static entries.
Nothing here shares code with the kernels or with unimedvl_amd.
"""
import numpy as np

TILE = 16
COUNT_MASK, CONTEXT, LISTED = 0x3FFFFFFF, 0x40000000, 0x80000000


def bf16_bits(x):
    """float32 array -> uint16 bf16 bit patterns, round to nearest even (NaN -> a quiet NaN of the same sign)"""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(np.asarray(x, dtype=np.float32))
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def bf16_float(bits):
    """uint16 bf16 bit patterns -> float32"""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def static_entries(context, bias):
    """(columns, bias values, in-context flags) of a row's static list entries"""
    cols, seen = [], set()
    for t in context or ():
        if int(t) not in seen:
            seen.add(int(t))
            cols.append(int(t))
    n_ctx = len(cols)
    for t in (bias or {}):
        if int(t) not in seen:
            seen.add(int(t))
            cols.append(int(t))
    return cols, [float((bias or {}).get(c, 0.0)) for c in cols], [i < n_ctx for i in range(len(cols))]


class History:
    """One row's penalty state.  n_static >= the row's static entries (the rest of the static section is -1), cap the list's capacity."""

    def __init__(self, V, cap, context=None, bias=None, n_static=None):
        cols, bvals, ctx = static_entries(context, bias)
        self.V, self.cap = V, cap
        self.n_static = len(cols) if n_static is None else n_static
        assert len(cols) <= self.n_static <= cap
        self.count = np.zeros(V, dtype=np.uint32)
        self.list = np.full(cap, -1, dtype=np.int32)
        self.bias = np.zeros(self.n_static, dtype=np.float32)
        for i, (c, b, x) in enumerate(zip(cols, bvals, ctx)):
            self.list[i] = c
            self.bias[i] = b
            self.count[c] = LISTED | (CONTEXT if x else 0)
        self.len = -1

    def copy(self):
        h = History.__new__(History)
        h.__dict__.update({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.__dict__.items()})
        return h

    def record(self, token):
        """what the kernel does with the token a step is fed, before it patches"""
        if self.len < 0:
            self.len = self.n_static
            return
        if not 0 <= token < self.V:
            return
        w = int(self.count[token])
        if (w & COUNT_MASK) != COUNT_MASK:
            w += 1
        if not (w & LISTED) and self.len < self.cap:
            self.list[self.len] = token
            self.len += 1
            w |= LISTED
        self.count[token] = w

    def entries(self):
        """(index, column) of the list entries the kernel visits"""
        return [(i, int(n)) for i, n in enumerate(self.list[:max(self.len, 0)]) if 0 <= n < self.V]


def adjust_row(bits, hist, r=1.0, presence=0.0, frequency=0.0):
    """uint16 [V] stored logits -> uint16 [V] adjusted logits for the row's history (after record)"""
    out = np.array(bits, dtype=np.uint16, copy=True)
    r, presence, frequency = np.float32(r), np.float32(presence), np.float32(frequency)
    with np.errstate(all="ignore"):
        for i, n in hist.entries():
            w = int(hist.count[n])
            c = w & COUNT_MASK
            l = bf16_float(out[n:n + 1])[0]
            a = l
            if (c > 0 or (w & CONTEXT)) and r != np.float32(1.0):
                a = np.float32(a * r) if a < 0 else np.float32(a / r)
            if c > 0:
                a = np.float32(a - np.float32(presence + np.float32(frequency * np.float32(c))))
            if i < hist.n_static and hist.bias[i] != 0:
                a = np.float32(a + hist.bias[i])
            if np.float32(a).view(np.uint32) != np.float32(l).view(np.uint32):
                out[n] = bf16_bits(np.array([a], dtype=np.float32))[0]
    return out


def same_bits(a, b):
    """bf16 bit patterns equal, any NaN equal to any NaN"""
    a, b = np.asarray(a, dtype=np.uint16), np.asarray(b, dtype=np.uint16)
    return (a == b) | (np.isnan(bf16_float(a)) & np.isnan(bf16_float(b)))


def greedy_keys(bits):
    """uint16 [V] -> uint64 [ceil(V / 16)]: per tile the maximum of (order-preserving image of the logit) << 32 | (0xFFFFFFFF - column):
    the largest logit, the lowest column among equals, -0 == +0, NaN highest"""
    v = bf16_float(bits)
    u = np.where(v == 0, np.float32(0), v).view(np.uint32).astype(np.uint64)
    k = np.where(np.isnan(v), np.uint64(0xFFFFFFFF), np.where(u & 0x80000000, ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000)))
    key = (k.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(len(v), dtype=np.uint64))
    nt = (len(v) + TILE - 1) // TILE
    pad = np.zeros(nt * TILE, dtype=np.uint64)
    pad[:len(v)] = key
    return pad.reshape(nt, TILE).max(axis=1)


def pick_values(bits, temperature=0.0):
    """uint16 [V] -> float64 [V]: y, the value the pick orders without noise: the logit, or bf16(float32(logit) / float32(T))"""
    v = bf16_float(bits)
    if temperature and temperature > 0:
        with np.errstate(all="ignore"):
            v = bf16_float(bf16_bits(v / np.float32(temperature)))
    return v.astype(np.float64)


def tile_stats(bits, temperature=0.0):
    """uint16 [V] -> (m, s) float64 [ceil(V / 16)]: per tile max y and sum exp(y - m); a tile of -inf only is (-inf, 0)"""
    y = pick_values(bits, temperature)
    nt = (len(y) + TILE - 1) // TILE
    pad = np.full(nt * TILE, -np.inf)
    pad[:len(y)] = y
    t = pad.reshape(nt, TILE)
    with np.errstate(all="ignore"):
        m = np.fmax.reduce(t, axis=1)
        ref = np.where(np.isneginf(m), 0.0, m)
        s = np.exp(t - ref[:, None]).sum(axis=1)
    return m, s


def logprob(bits, token, temperature=0.0):
    """float64 log-probability of `token` under softmax(y) of the row"""
    y = pick_values(bits, temperature)
    with np.errstate(all="ignore"):
        m = np.max(y)
        m = m if np.isfinite(m) else 0.0
        return float(y[token] - (m + np.log(np.exp(y - m).sum())))
