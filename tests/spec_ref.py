"""Plain-Python model of umv_decode_step_end_speculative (include/unimedvl_hip.h, "speculative greedy decode"): steps 1-8 of one
sample on Python ints and lists.  The GPU tests hold every output word of the kernel to it; the CPU tests drive it with a toy model."""
import math


def lookup(hist, k, ngram_min, ngram_max, vocab):
    """Prompt-lookup drafts for a history (a list of ints, negative entries are separators): the first g from ngram_max down to
    ngram_min whose suffix occurs earlier decides, at its most recent occurrence; the drafts are what followed it."""
    n = len(hist)
    for g in range(ngram_max, ngram_min - 1, -1):
        if n <= g:
            continue
        suf = hist[n - g:]
        if any(t < 0 for t in suf):
            continue
        for i in range(n - g - 1, -1, -1):
            if hist[i:i + g] == suf:
                out = []
                for j in range(1, k + 1):
                    at = i + g + j - 1
                    if at >= n or not 0 <= hist[at] < vocab:
                        break
                    out.append(hist[at])
                return out
    return []


def from_predicted(predicted, pred_len, n_out, k, vocab):
    out = []
    for j in range(1, k + 1):
        at = n_out + j - 1
        if at >= pred_len or at >= len(predicted) or not 0 <= predicted[at] < vocab:
            break
        out.append(predicted[at])
    return out


class Sample:
    """The words of one sample: rows (ids / tok_slot / tok_pos of its k + 1 rows), kv_len, out (the out_ids row), n_out, limit,
    n_draft, hist (a list of hist_ld entries) / hist_len, predicted / pred_len, stats."""

    def __init__(self, k, t0, slot, pos, out_ld, limit, hist, hist_ld, vocab, ngram=(2, 4), predicted=None, pred_len=0):
        self.k, self.vocab, self.ngram = k, vocab, tuple(ngram)
        self.ids = [t0] * (k + 1)
        self.tok_slot = [slot + j for j in range(k + 1)]
        self.tok_pos = [pos + j for j in range(k + 1)]
        self.kv_len = slot + k + 1
        self.out = [0] * out_ld
        self.n_out, self.limit, self.n_draft = 0, limit, 0
        self.hist = list(hist) + [0] * (hist_ld - len(hist))
        self.hist_len = len(hist)
        self.predicted, self.pred_len = (None if predicted is None else list(predicted)), pred_len
        self.stats = [0, 0, 0]

    def draft(self):
        """steps 6 and 7 (the draft_only call)"""
        k = self.k
        if self.predicted is not None and self.pred_len > 0:
            d = from_predicted(self.predicted, self.pred_len, self.n_out, k, self.vocab)
        else:
            d = lookup(self.hist[:self.hist_len], k, self.ngram[0], self.ngram[1], self.vocab)
        t0 = self.ids[0]
        self.ids = [t0] + d + [t0] * (k - len(d))
        self.tok_slot = [self.tok_slot[0] + j for j in range(k + 1)]
        self.tok_pos = [self.tok_pos[0] + j for j in range(k + 1)]
        self.n_draft = len(d)

    def step_end(self, picks):
        """steps 1-8 given the k + 1 picks p_0..p_k; returns (n, m)"""
        k = self.k
        assert len(picks) == k + 1
        n = 0
        while n < self.n_draft and n < k and self.ids[n + 1] == picks[n]:
            n += 1
        lim = min(self.limit, len(self.out))
        m = max(0, min(n + 1, lim - self.n_out))
        for i in range(m):
            self.out[self.n_out + i] = picks[i]
            if self.hist_len < len(self.hist):
                self.hist[self.hist_len] = picks[i]
                self.hist_len += 1
        self.n_out += m
        self.kv_len += m
        self.tok_slot[0] += m
        self.tok_pos[0] += m
        if m > 0:
            self.ids[0] = picks[m - 1]
        self.stats = [self.stats[0] + 1, self.stats[1] + self.n_draft, self.stats[2] + n]
        self.draft()
        return n, m


def plain_greedy(next_token, context, t0, count):
    """`count` tokens of plain greedy decoding: next_token(sequence) -> token, the sequence being context + [t0] + what was generated"""
    seq, out = list(context) + [t0], []
    for _ in range(count):
        out.append(next_token(seq))
        seq.append(out[-1])
    return out


def run(sample, next_token, context, max_steps=None, redraft=None):
    """Drive a Sample with a toy model to its limit: row j's pick is next_token(context + [first input] + emitted + rows 0..j).
    redraft(sample): optional, rewrites the drafted rows (ids[1:], n_draft) before each step - adversarial drafts.  Returns steps."""
    first = sample.ids[0]
    steps = 0
    max_steps = max_steps if max_steps is not None else 4 * sample.limit + 4
    while sample.n_out < min(sample.limit, len(sample.out)) and steps < max_steps:
        if redraft is not None:
            redraft(sample)
        base = list(context) + [first] + sample.out[:sample.n_out]
        assert base[-1] == sample.ids[0]
        picks = [next_token(base + sample.ids[1:j + 1]) for j in range(sample.k + 1)]
        sample.step_end(picks)
        steps += 1
    return steps


def steps_for(tokens, k):
    return math.ceil(tokens / (k + 1))
