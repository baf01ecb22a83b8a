"""The definition of the banned-sequence stage (include/unimedvl_hip.h, "banned sequences") in plain Python: the state a row owns
(count and tail), the record step of umv_logit_sequence_ban_bf16, the banned set of a table, the banned row, and the beam form's walk
over the back-pointers.  Everything here is integer work, so a kernel result is compared with it bit for bit.

A table is a list of entries (tokens, until): `tokens` a list of 1..SEQ_MAX ints, `until` 0, a positive int or ROW."""
import numpy as np

SEQ_MAX = 16            # UMV_SEQ_MAX
TAIL = SEQ_MAX - 1      # history words a row keeps
ROW = -1                # UMV_SEQ_ROW
NINF = 0xFF80           # bf16 -inf
COUNT_MAX = (1 << 31) - 1


class State:
    """one row's words: count (negative = the row is off) and tail (int32 [TAIL], most recent last, -1 where there is none)"""

    def __init__(self, fed=(), count=None):
        self.count = 0
        self.tail = np.full(TAIL, -1, dtype=np.int32)
        for t in fed:
            self.record(t)
        if count is not None:
            self.count = int(count)

    def copy(self):
        s = State()
        s.count, s.tail = self.count, self.tail.copy()
        return s

    def record(self, token):
        """the kernel's record step for the token the step is fed"""
        if self.count < 0:
            return
        token = int(token)
        self.tail[:-1] = self.tail[1:]
        self.tail[-1] = token if 0 <= token < 1 << 31 else -1
        self.count = min(self.count + 1, COUNT_MAX)


def active(until, count, row_min=None):
    """is an entry with this `until` word active for a row with `count` tokens fed?"""
    if until == 0:
        return True
    if until > 0:
        return count <= until
    if until == ROW:
        return row_min is not None and count <= row_min
    return False


def banned(table, count, tail, V, row_min=None):
    """The banned set, sorted: the definition, entry by entry.  tail: the last TAIL tokens fed, most recent last."""
    tail = [int(t) for t in tail]
    out = set()
    if count < 0:
        return []
    for tokens, until in table:
        m = len(tokens)
        if not 1 <= m <= SEQ_MAX or not active(until, count, row_min) or m - 1 > count:
            continue
        last = tail[TAIL - (m - 1):] if m > 1 else []
        if any(not 0 <= h < V for h in last) or last != [int(t) for t in tokens[:m - 1]]:
            continue
        if 0 <= tokens[m - 1] < V:
            out.add(int(tokens[m - 1]))
    return sorted(out)


def ban_row(bits, cols):
    """bf16 bit patterns (uint16 [V]) of a row with `cols` banned"""
    out = np.array(bits, dtype=np.uint16, copy=True)
    out[list(cols)] = NINF
    return out


def step(bits, state, token, table, row_min=None):
    """One plain-form kernel call on one row: record `token` in state (updated in place), then ban.  Returns (bits, banned columns)."""
    state.record(token)
    cols = banned(table, state.count, state.tail, len(bits), row_min)
    return ban_row(bits, cols), cols


def history_state(fed):
    """(count, tail) of a row that was fed the tokens `fed` since its slot started: what the plain form holds after recording them"""
    s = State(fed)
    return s.count, s.tail


def beam_state(beam_tok, beam_parent, t, r, K, fed, start, max_m):
    """The beam form's (count, tail) of row r = b * K + i at step t: count = t + 1; the tail is `fed` (ids[r]), then
    beam_tok[u][b * K + i_u] for u = t - 2, t - 3, ... with i_{t-2} = beam_parent[t - 1][r], i_{u-1} = beam_parent[u][b * K + i_u], then
    the request's start token - max_m - 1 tokens in all, -1 beyond.  beam_tok / beam_parent: [max_len][R]."""
    tail = np.full(TAIL, -1, dtype=np.int32)
    max_len = len(beam_tok)
    if not 0 <= t < max_len:
        return -1, tail
    word = lambda v: int(v) if 0 <= int(v) < 1 << 31 else -1
    need = max_m - 1
    base, beam = r - r % K, r % K
    if need >= 1:
        tail[TAIL - 1] = word(fed)
    for d in range(1, need):
        pos = t - d
        if pos < 0:
            break
        if pos == 0:
            tail[TAIL - 1 - d] = word(start)
            break
        beam = int(beam_parent[pos][base + beam])
        if not 0 <= beam < K:
            break
        tail[TAIL - 1 - d] = int(beam_tok[pos - 1][base + beam])
    return t + 1, tail


def beam_step(bits, beam_tok, beam_parent, t, r, K, fed, start, table, max_m, row_min=None):
    """One beam-form kernel call on one row.  Returns (bits, banned columns)."""
    count, tail = beam_state(beam_tok, beam_parent, t, r, K, fed, start, max_m)
    cols = banned(table, count, tail, len(bits), row_min)
    return ban_row(bits, cols), cols


def table_of(seq_ptr, seq_tok, seq_until):
    """the CSR arrays of ops.sequence_table as a table of this module"""
    return [([int(v) for v in seq_tok[seq_ptr[s]:seq_ptr[s + 1]]], int(seq_until[s])) for s in range(len(seq_until))]
