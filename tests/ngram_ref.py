"""The definition of no_repeat_ngram_size (include/unimedvl_hip.h, "no-repeat n-grams") in plain Python: the history record of
umv_logit_ngram_ban_bf16 and the banned set, on lists and numpy arrays.  Everything here is integer work, so a kernel result is
compared with it bit for bit."""
import numpy as np

NGRAM_MAX = 16          # UMV_NGRAM_MAX
FULL = -2               # UMV_NGRAM_FULL
NINF = 0xFF80           # bf16 -inf


class History:
    """one row's history: hist (int32 [hist_ld]) and its length word (negative = the row is off)"""

    def __init__(self, hist_ld, context=(), length=None):
        self.hist = np.zeros(hist_ld, dtype=np.int32)
        context = [int(t) for t in context]
        self.hist[:len(context)] = context
        self.len = len(context) if length is None else int(length)

    def copy(self):
        h = History(len(self.hist))
        h.hist, h.len = self.hist.copy(), self.len
        return h

    def record(self, token):
        """the kernel's record step for the token the step is fed"""
        if self.len < 0:
            return
        if self.len >= len(self.hist):
            self.len = FULL
            return
        token = int(token)
        self.hist[self.len] = token if 0 <= token < 1 << 31 else -1
        self.len += 1

    def tokens(self):
        return [] if self.len < 0 else self.hist[:self.len].tolist()


def banned(h, n, V):
    """The banned set of history h (a list of ints) at size n over V columns, sorted: the definition, candidate by candidate."""
    L = len(h)
    if not 1 <= n <= NGRAM_MAX or L < n:
        return []
    suffix = h[L - n + 1:]
    if any(not 0 <= t < V for t in suffix):
        return []
    out = set()
    for i in range(L - n + 1):
        if h[i:i + n - 1] == suffix and 0 <= h[i + n - 1] < V:
            out.add(h[i + n - 1])
    return sorted(out)


def banned_table(h, n, V):
    """The same set a second way - the table HF's processor builds: every n-gram of h keyed by its first n - 1 tokens, looked up with
    the last n - 1 tokens; an n-gram that holds an entry outside [0, V) in its key is no key anyone can look up."""
    L = len(h)
    if not 1 <= n <= NGRAM_MAX or L < n:
        return []
    table = {}
    for i in range(L - n + 1):
        gram = tuple(h[i:i + n])
        table.setdefault(gram[:-1], []).append(gram[-1])
    key = tuple(h[L - n + 1:])
    if any(not 0 <= t < V for t in key):
        return []
    return sorted({t for t in table.get(key, []) if 0 <= t < V})


def ban_row(bits, h, n):
    """bf16 bit patterns (uint16 [V]) of a row after the ban of history h (a list) at size n, and the banned columns"""
    out = np.array(bits, dtype=np.uint16, copy=True)
    cols = banned(h, n, len(out))
    out[cols] = NINF
    return out, cols


def step(bits, hist, token, n):
    """One kernel call on one row: record `token` in hist (a History, updated in place), then ban.  Returns (bits, banned columns)."""
    hist.record(token)
    if hist.len < 0:
        return np.array(bits, dtype=np.uint16, copy=True), []
    return ban_row(bits, hist.tokens(), n)
