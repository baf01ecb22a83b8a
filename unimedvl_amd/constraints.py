"""Token automata for constrained decoding (include/unimedvl_hip.h, "token automata").

A TokenAutomaton says which tokens a request may be fed next, as a function of what it was fed so far: a deterministic automaton over
token ids, kept in CSR form (numpy int32) on the host and copied to the device once.  State s owns the edges row_ptr[s] ..
row_ptr[s + 1] - 1, sorted by token; edge_next is the state after that token, FREE (-1) releases the request.  The decode step masks
the logits of a row to the tokens of its state's edges (umv_logit_constrain_bf16) and moves the row's state word along the edge of the
token it is fed (umv_constraint_advance) - `walk` is the host model of that second kernel.

    a = TokenAutomaton.from_choices([tok("yes"), tok("no")], eos_id)          # one of the answers, then EOS
    a = TokenAutomaton.from_choices([tok("Findings:")], None, after="free")    # a fixed prefix, then free text
    a = TokenAutomaton.from_allowed_tokens(digits)                             # any sequence over a token set
    merged, start = TokenAutomaton.union({"yn": a1, "abcd": a2})               # one table, each member's start state
"""
import numpy as np

FREE = -1       # UMV_CONSTRAINT_FREE: the row is unconstrained
LEFT = -2       # UMV_CONSTRAINT_LEFT: the row was fed a token its state has no edge for; unconstrained from then on


def _token(t, what="token"):
    if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, np.integer)) or t < 0 or t > 0x7FFFFFFF:
        raise ValueError(f"{what} {t!r} is not an integer in [0, 2^31)")
    return int(t)


class TokenAutomaton:
    def __init__(self, row_ptr, edge_token, edge_next, allow_empty_states=False):
        """Takes the three CSR arrays and validates them: row_ptr [n_states + 1] ascending from 0 to the edge count, the tokens of
        every state strictly ascending (sorted, distinct) and >= 0, edge_next in [-1, n_states).  A state without edges is legal for
        the kernels (it masks every column) and nothing a user wants: ValueError unless allow_empty_states."""
        def arr(a, name):
            a = np.asarray(a)
            if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
                raise ValueError(f"{name} must be a one-dimensional integer array")
            a = a.astype(np.int64)
            if a.size and (a.min() < -(1 << 31) or a.max() > 0x7FFFFFFF):
                raise ValueError(f"{name} does not fit int32")
            return np.ascontiguousarray(a.astype(np.int32))
        self.row_ptr, self.edge_token, self.edge_next = arr(row_ptr, "row_ptr"), arr(edge_token, "edge_token"), arr(edge_next, "edge_next")
        rp, tok, nxt = self.row_ptr, self.edge_token, self.edge_next
        if rp.size < 2:
            raise ValueError("an automaton has at least one state (row_ptr holds n_states + 1 entries)")
        if tok.size != nxt.size:
            raise ValueError(f"edge_token ({tok.size}) and edge_next ({nxt.size}) must hold one entry per edge")
        if rp[0] != 0 or rp[-1] != tok.size or (np.diff(rp) < 0).any():
            raise ValueError("row_ptr must ascend from 0 to the number of edges")
        n = self.n_states
        if tok.size and tok.min() < 0:
            raise ValueError("edge_token holds a negative token")
        if nxt.size and (nxt.min() < FREE or nxt.max() >= n):
            raise ValueError(f"edge_next must lie in [-1, {n}) (-1 = FREE)")
        inner = np.ones(tok.size, dtype=bool)           # edges that are not the first of their state
        inner[rp[:-1][rp[:-1] < tok.size]] = False
        if tok.size and (np.diff(tok.astype(np.int64), prepend=-1)[inner] <= 0).any():
            raise ValueError("the edge tokens of a state must be strictly ascending (sorted, distinct)")
        if not allow_empty_states and (np.diff(rp) == 0).any():
            raise ValueError(f"state {int(np.flatnonzero(np.diff(rp) == 0)[0])} has no edge: it would mask every token")

    n_states = property(lambda self: int(self.row_ptr.size - 1))
    n_edges = property(lambda self: int(self.edge_token.size))

    # ---- builders
    @classmethod
    def _from_edges(cls, edges, **kw):
        """edges: per state a {token: next state} mapping"""
        row_ptr, tok, nxt = [0], [], []
        for e in edges:
            for t in sorted(e):
                tok.append(t)
                nxt.append(e[t])
            row_ptr.append(len(tok))
        return cls(row_ptr, np.array(tok, dtype=np.int64), np.array(nxt, dtype=np.int64), **kw)

    @classmethod
    def from_choices(cls, choices, eos_id, after="stop"):
        """The request emits exactly one of `choices` (token-id sequences), from state 0: a trie, common prefixes shared.
        after="stop": the end of a choice is followed by eos_id, into a final state whose only edge is an eos_id self-loop - a row that
        keeps stepping until the host harvests it stays well-defined.  One choice may be a prefix of another: that state has both the
        EOS edge and the continuation.  after="free": the last token of a choice releases the row (FREE) - free text follows; eos_id is
        not used (None is fine) and no choice may be a prefix of another, since the row cannot both go on and be released.
        Empty and duplicate choices raise, and so does a choice that holds eos_id under after="stop"."""
        if after not in ("stop", "free"):
            raise ValueError(f"after must be 'stop' or 'free', got {after!r}")
        seqs = [[_token(t, "choice token") for t in (c.tolist() if hasattr(c, "tolist") else c)] for c in choices]
        if not seqs:
            raise ValueError("from_choices needs at least one choice")
        if any(not s for s in seqs):
            raise ValueError("an empty choice")
        if len({tuple(s) for s in seqs}) != len(seqs):
            raise ValueError("duplicate choices")
        eos = None
        if after == "stop":
            eos = _token(eos_id, "eos_id")
            if any(eos in s for s in seqs):
                raise ValueError(f"a choice holds eos_id ({eos})")
        edges, ends = [{}], set()
        for s in seqs:
            at = 0
            for t in s:
                if t not in edges[at]:
                    edges.append({})
                    edges[at][t] = len(edges) - 1
                at = edges[at][t]
            ends.add(at)
        if after == "stop":
            final = len(edges)
            edges.append({eos: final})
            for s in ends:
                edges[s][eos] = final
            return cls._from_edges(edges)
        if any(edges[s] for s in ends):
            raise ValueError("after='free': a choice is a prefix of another - the row cannot both go on and be released")
        # the end states have no edge and nothing leads anywhere from them: point their incoming edges at FREE and drop them
        keep = [s for s in range(len(edges)) if s not in ends]
        number = {s: i for i, s in enumerate(keep)}
        return cls._from_edges([{t: number.get(n, FREE) for t, n in edges[s].items()} for s in keep])

    @classmethod
    def from_allowed_tokens(cls, ids):
        """Any sequence over the token set `ids`: one state with a self-loop per token"""
        toks = sorted({_token(t, "allowed token") for t in (ids.tolist() if hasattr(ids, "tolist") else ids)})
        if not toks:
            raise ValueError("from_allowed_tokens needs at least one token")
        return cls._from_edges([{t: 0 for t in toks}])

    @classmethod
    def union(cls, named):
        """{name: TokenAutomaton} -> (one automaton holding every member, {name: the member's state 0 in it}).  The members do not
        share states; a row started in a member's start state never leaves that member."""
        if not named:
            raise ValueError("union needs at least one automaton")
        rp, tok, nxt, start = [np.zeros(1, dtype=np.int64)], [], [], {}
        states = edges = 0
        for name, a in named.items():
            if not isinstance(a, TokenAutomaton):
                raise ValueError(f"union: {name!r} is not a TokenAutomaton")
            start[name] = states
            rp.append(a.row_ptr[1:].astype(np.int64) + edges)
            tok.append(a.edge_token.astype(np.int64))
            nxt.append(np.where(a.edge_next >= 0, a.edge_next.astype(np.int64) + states, a.edge_next))
            states += a.n_states
            edges += a.n_edges
        return cls(np.concatenate(rp), np.concatenate(tok), np.concatenate(nxt), allow_empty_states=True), start

    # ---- the host model
    def is_free(self, state):
        return state < 0 or state >= self.n_states

    def allowed(self, state):
        """the tokens a row in `state` may be fed (int32, ascending); None for a free row"""
        if self.is_free(state):
            return None
        return self.edge_token[self.row_ptr[state]:self.row_ptr[state + 1]].copy()

    def step(self, state, token):
        """umv_constraint_advance for one row: a free row keeps its word, a token without an edge gives LEFT"""
        if self.is_free(state):
            return int(state)
        lo, hi = int(self.row_ptr[state]), int(self.row_ptr[state + 1])
        e = lo + int(np.searchsorted(self.edge_token[lo:hi], token))
        return int(self.edge_next[e]) if e < hi and int(self.edge_token[e]) == int(token) else LEFT

    def walk(self, start, tokens, trace=False):
        """the state after feeding `tokens` from `start` (trace=True: the state after every token, as a list)"""
        s, seen = int(start), []
        for t in tokens:
            s = self.step(s, int(t))
            seen.append(s)
        return seen if trace else s

    def to_device(self, device):
        """The tables in device memory, for ops.logit_constrain / ops.constraint_advance and DecodeSession(constraint=)"""
        return DeviceAutomaton(self, device)


class DeviceAutomaton:
    """A TokenAutomaton's three tables as int32 tensors on one device; `host` is the automaton they were copied from."""

    def __init__(self, host, device):
        import torch
        self.host = host
        self.n_states, self.n_edges = host.n_states, host.n_edges
        self.row_ptr = torch.from_numpy(host.row_ptr).to(device)
        self.edge_token = torch.from_numpy(host.edge_token).to(device)
        self.edge_next = torch.from_numpy(host.edge_next).to(device)

    @property
    def device(self):
        return self.row_ptr.device
