"""numpy restatement of constrained decoding (include/unimedvl_hip.h, "token automata") for the tests.

An automaton is three integer arrays in CSR form: state s owns the edges row_ptr[s] .. row_ptr[s + 1] - 1, edge e carries the token
edge_token[e] and the next state edge_next[e].  A row's state word that is negative or >= n_states marks a free row.

    masked row:  columns outside A = {tokens of the state's edges in [0, V)} become bf16 -inf (0xFF80), columns in A keep their bits
    free row:    unchanged
    advance:     a free row keeps its word; otherwise the word becomes the next state of the edge for the fed token, LEFT if none

Keys, statistics and log-probabilities of a masked row are those of tests/penalty_ref.py on the masked bits (greedy_keys, pick_values,
tile_stats, logprob).  Nothing here shares code with the kernels or with unimedvl_amd: the edge lists are scanned, not searched.
"""
import numpy as np

import penalty_ref as P

NEG_INF = 0xFF80
FREE, LEFT = -1, -2
TILE = P.TILE


class Automaton:
    def __init__(self, row_ptr, edge_token, edge_next):
        self.row_ptr = [int(v) for v in row_ptr]
        self.edge_token = [int(v) for v in edge_token]
        self.edge_next = [int(v) for v in edge_next]
        self.n_states = len(self.row_ptr) - 1

    @classmethod
    def from_states(cls, states):
        """states: per state a list of (token, next state) pairs, in any order"""
        row_ptr, tok, nxt = [0], [], []
        for edges in states:
            for t, n in sorted(edges):
                tok.append(t)
                nxt.append(n)
            row_ptr.append(len(tok))
        return cls(row_ptr, tok, nxt)

    def arrays(self):
        return (np.array(self.row_ptr, dtype=np.int32), np.array(self.edge_token, dtype=np.int32), np.array(self.edge_next, dtype=np.int32))

    def free(self, s):
        return s < 0 or s >= self.n_states

    def edges(self, s):
        return [(self.edge_token[e], self.edge_next[e]) for e in range(self.row_ptr[s], self.row_ptr[s + 1])]

    def allowed(self, s, V):
        """the allowed columns of a row in state s, ascending; None for a free row"""
        if self.free(s):
            return None
        return sorted(t for t, _ in self.edges(s) if 0 <= t < V)

    def step(self, s, token):
        if self.free(s):
            return s
        for t, n in self.edges(s):
            if t == token:
                return n
        return LEFT

    def walk(self, s, tokens):
        """the state after every token"""
        out = []
        for t in tokens:
            s = self.step(s, int(t))
            out.append(s)
        return out


def mask_row(bits, automaton, s):
    """uint16 [V] stored logits -> uint16 [V] masked logits of a row in state s (a copy; a free row's own bits)"""
    out = np.array(bits, dtype=np.uint16, copy=True)
    A = automaton.allowed(s, len(out))
    if A is None:
        return out
    keep = np.zeros(len(out), dtype=bool)
    keep[A] = True
    out[~keep] = NEG_INF
    return out


def greedy_keys(bits):
    return P.greedy_keys(bits)


def tile_stats(bits, temperature=0.0):
    return P.tile_stats(bits, temperature)


def logprob(bits, token, temperature=0.0):
    return P.logprob(bits, token, temperature)


def restricted_logprob(bits, A, token, temperature=0.0):
    """fp64 log-softmax over the columns A alone of y (P.pick_values) of the UNMASKED row: what the masked row's logprob must equal"""
    y = P.pick_values(bits, temperature)[np.array(A, dtype=np.int64)]
    with np.errstate(all="ignore"):
        m = np.max(y)
        m = m if np.isfinite(m) else 0.0
        return float(P.pick_values(bits, temperature)[token] - (m + np.log(np.exp(y - m).sum())))


def restricted_argmax(bits, A):
    """the lowest column among the largest logits of A (NaN highest, -0 == +0): the greedy pick of the masked row.  Where every
    allowed logit is -inf the masked row is a row of -inf only, and its pick is what such a row's pick is: column 0."""
    v = P.bf16_float(bits)
    if all(v[n] == -np.inf for n in A):
        return 0
    best, at = None, -1
    for n in A:
        x = v[n]
        rank = (2, 0.0) if np.isnan(x) else (1, float(x))
        if best is None or rank > best:
            best, at = rank, n
    return at
