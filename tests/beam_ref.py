"""Plain-Python form of beam search decode (include/unimedvl_hip.h, "beam search decode"): the candidate lists, the step end
(umv_beam_step_end) word for word - order, walk, finished list, done rule, counters, page-table rows and copy list - and the whole
search over a model given as a function  prefixes -> log-prob rows,  so that it knows nothing of the engine.  Every score is fp32:
numpy float32 scalars add and divide as the device does (one rounding each), so the tests compare bits."""
import numpy as np

F = np.float32
NEG = F(-np.inf)
PAGE = 256


def length_norm(max_length, length_penalty):
    """norm[t] = powf(t + 1, length_penalty) in fp32: the table the host hands the step end (a hypothesis that ends at step t has
    t + 1 generated tokens, the end token counted)"""
    return np.power(np.arange(1, max_length + 1, dtype=np.float32), F(length_penalty)).astype(np.float32)


def top_candidates(lp_row, n):
    """the first n columns of a log-prob row by (value descending, column ascending): (ids int32 [n], lp fp32 [n])"""
    lp_row = np.asarray(lp_row, dtype=np.float32)
    order = np.lexsort((np.arange(lp_row.size), -lp_row.astype(np.float64)))[:n]
    return order.astype(np.int32), lp_row[order]


class Request:
    """the words one request owns on the device"""

    def __init__(self, K, max_length, end_token_id, length_penalty=1.0, early_stopping=False):
        self.K, self.max_length, self.end = int(K), int(max_length), -1 if end_token_id is None else int(end_token_id)
        self.early = bool(early_stopping)
        self.norm = length_norm(max_length, length_penalty)
        self.scores = np.full(K, NEG, dtype=np.float32)
        self.scores[0] = F(0)
        self.n_fin = self.n_ever = self.done = 0
        # finished list: slot -> (score, total, lp of the last token) and (step, parent beam, last token, sequence number)
        self.fin_f = np.zeros((K, 4), dtype=np.float32)
        self.fin_i = np.zeros((K, 4), dtype=np.int32)
        self.tok = np.zeros((max_length, K), dtype=np.int32)
        self.parent = np.zeros((max_length, K), dtype=np.int32)
        self.lp = np.zeros((max_length, K), dtype=np.float32)
        self.steps = 0
        self.reached = set()             # which branches a step took (the crafted tests assert the case was reached)

    def _offer(self, score, total, lp, t, parent, tok):
        K = self.K
        if self.n_fin < K:
            slot = self.n_fin
            self.n_fin += 1
            self.reached.add("append")
        else:
            slot = 0                     # the worst: lowest score, the latest entry among equals
            for i in range(1, K):
                if self.fin_f[i, 0] < self.fin_f[slot, 0] or (self.fin_f[i, 0] == self.fin_f[slot, 0] and self.fin_i[i, 3] > self.fin_i[slot, 3]):
                    slot = i
            if not score > self.fin_f[slot, 0]:
                self.reached.add("equal_kept" if score == self.fin_f[slot, 0] else "worse_kept")
                return
            self.reached.add("replace")
        self.fin_f[slot] = (score, total, lp, 0)
        self.fin_i[slot] = (t, parent, tok, self.n_ever)
        self.n_ever += 1

    def step_end(self, cand_ids, cand_lp):
        """One step end over the K rows' candidate lists ([K][2K]).  Returns None for a done request (no word is written), else
        (tokens, parents, totals, lps) of the next live beams - what the step wrote to ids / beam_tok / beam_parent / scores / beam_lp."""
        if self.done:
            self.reached.add("done_untouched")
            return None
        K, t = self.K, self.steps
        cands = []
        for i in range(K):
            if not self.scores[i] > NEG:                 # a beam at -inf (or NaN) contributes nothing
                self.reached.add("dead_beam")
                continue
            for j in range(cand_ids.shape[1]):
                total = F(self.scores[i] + F(cand_lp[i, j]))
                if cand_ids[i, j] < 0 or total != total:
                    continue
                cands.append((total, i, j))
        cands.sort(key=lambda c: (-float(c[0]), c[1], c[2]))
        last = t + 1 == self.max_length
        live = []
        for r, (total, i, j) in enumerate(cands):
            tok, lp = int(cand_ids[i, j]), F(cand_lp[i, j])
            is_end = tok == self.end
            if r < K and (is_end or last):
                self.reached.add("end_top" if is_end else "max_length")
                self._offer(F(total / self.norm[t]), total, lp, t, i, tok)
            elif is_end:
                self.reached.add("end_skipped")
            if not is_end and len(live) < K:
                live.append((tok, i, total, lp))
            if len(live) == K and r >= K - 1:
                break
        while len(live) < K:                             # fewer than K candidates in all (NaN rows): dead successors
            live.append((0, len(live), NEG, NEG))
        full = self.n_fin == K
        if self.early:
            self.done = int(full)
        else:
            worst = min(float(self.fin_f[i, 0]) for i in range(K)) if full else 0.0
            self.done = int(full and F(worst) >= F(live[0][2] / self.norm[t]))
            if full:
                self.reached.add("heuristic_done" if self.done else "heuristic_open")
        toks, parents, totals, lps = (np.array(v) for v in zip(*live))
        self.tok[t], self.parent[t], self.lp[t] = toks, parents, lps.astype(np.float32)
        self.scores = totals.astype(np.float32)
        self.steps += 1
        return toks.astype(np.int64), parents.astype(np.int32), self.scores.copy(), lps.astype(np.float32)

    # ---- the host side: sequences from the back-pointers
    def hypotheses(self):
        """the finished list, best first (score descending, the earlier entry among equals): dicts with tokens (the last one
        included), tokens_no_end, score, total, logprobs"""
        out = []
        order = sorted(range(self.n_fin), key=lambda s: (-float(self.fin_f[s, 0]), int(self.fin_i[s, 3])))
        for s in order:
            t, parent, tok, _ = (int(v) for v in self.fin_i[s])
            toks, lps = [tok], [float(self.fin_f[s, 2])]
            beam = parent
            for u in range(t - 1, -1, -1):
                toks.append(int(self.tok[u, beam]))
                lps.append(float(self.lp[u, beam]))
                beam = int(self.parent[u, beam])
            toks.reverse()
            lps.reverse()
            out.append(dict(tokens=toks, tokens_no_end=toks[:-1] if toks[-1] == self.end else toks, score=float(self.fin_f[s, 0]),
                            total=float(self.fin_f[s, 1]), logprobs=lps))
        return out

    def live_prefixes(self):
        """the token lists of the K live beams after `steps` steps"""
        out = []
        for b in range(self.K):
            toks, beam = [], b
            for u in range(self.steps - 1, -1, -1):
                toks.append(int(self.tok[u, beam]))
                beam = int(self.parent[u, beam])
            out.append(toks[::-1])
        return out


def kv_plan(table, own, j0, L, parents, done_now=False):
    """The reorder rule for one request: table [K][P] (its rows of the page table before the step), own [K][NP][2] (the two private
    pages of every row and page index j0 + q), L the committed length after the step, parents [K].  Returns (new table, copy list
    [K][3] of (source page, destination page, tokens))."""
    K = len(parents)
    new = np.array(table, copy=True)
    copies = np.zeros((K, 3), dtype=np.int32)
    if done_now:
        return new, copies
    Lp, rem = L // PAGE, L % PAGE
    for c in range(K):
        p = int(parents[c])
        new[c, j0:Lp] = table[p, j0:Lp]
        q = Lp - j0
        if rem and p != c and q < own.shape[1]:
            cur = int(table[c, Lp])
            spare = int(own[c, q, 1]) if int(own[c, q, 0]) == cur else int(own[c, q, 0])
            copies[c] = (int(table[p, Lp]), spare, (rem + 7) // 8 * 8)
            new[c, Lp] = spare
    return new, copies


def search(model_fn, K, max_length, end_token_id, length_penalty=1.0, early_stopping=False, n_candidates=None):
    """The whole search of one request.  model_fn(prefixes) takes the K live beams' generated tokens (K lists) and returns their
    next-token log-probabilities [K][V] (fp32).  Returns the Request (hypotheses() is the result)."""
    req = Request(K, max_length, end_token_id, length_penalty, early_stopping)
    n = 2 * K if n_candidates is None else n_candidates
    while req.steps < max_length and not req.done:
        rows = np.asarray(model_fn(req.live_prefixes()), dtype=np.float32)
        ids, lps = zip(*(top_candidates(rows[i], n) for i in range(K)))
        req.step_end(np.stack(ids), np.stack(lps))
    return req
