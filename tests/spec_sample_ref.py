"""Plain-Python model of a sampled speculative step (include/unimedvl_hip.h, "speculative decode with sampling"): spec_ref.Sample
extended by the draw counters of the sample's table rows (step 9) and the copy of the emitted tokens' log-probabilities - the
definition of umv_decode_step_end_speculative_rows - and a host restatement of the sampler's noise (csrc/token_pick.h) in fp64."""
import math

import spec_ref as S

MASK = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def row_key(seed, draw, stream):
    """the key of a row: splitmix64(seed ^ draw * 0xD1B54A32D192ED03 ^ stream << 32)"""
    return splitmix64((seed & MASK) ^ ((draw * 0xD1B54A32D192ED03) & MASK) ^ ((stream << 32) & MASK))


def uniform(key, n):
    """u of column n: ((splitmix64(key + n) >> 41) + 0.5) * 2^-23, strictly inside (0, 1)"""
    return ((splitmix64((key + n) & MASK) >> 41) + 0.5) * 2.0 ** -23


def gumbel(key, n):
    return -math.log(-math.log(uniform(key, n)))


def gumbels(seed, draw, stream, V):
    key = row_key(seed, draw, stream)
    return [gumbel(key, n) for n in range(V)]


class Sample(S.Sample):
    """spec_ref.Sample plus draws (the draw counters of the sample's k + 1 table rows) and out_lp (the out_logprobs row)"""

    def __init__(self, *a, draw0=0, **kw):
        super().__init__(*a, **kw)
        self.draws = [draw0 + j for j in range(self.k + 1)]
        self.out_lp = [0.0] * len(self.out)

    def step_end(self, picks, row_logprob=None):
        """steps 1-9 given the picks p_0..p_k (and their log-probabilities); returns (n, m)"""
        before, d0 = self.n_out, self.draws[0]
        n, m = super().step_end(picks)
        if row_logprob is not None:
            for i in range(m):
                self.out_lp[before + i] = row_logprob[i]
        if m > 0:
            self.draws = [d0 + m + j for j in range(self.k + 1)]
        return n, m


def plain_sampled(pick, context, t0, count):
    """`count` tokens of the plain per-row session: t_i = pick(sequence, i), the sequence being context + [t0] + t_<i, i the draw"""
    seq, out = list(context) + [t0], []
    for i in range(count):
        out.append(pick(seq, i))
        seq.append(out[-1])
    return out


def run(sample, pick, context, max_steps=None, redraft=None):
    """spec_ref.run with a pick function of (sequence, draw): row j picks with the draw counter its table row holds"""
    first = sample.ids[0]
    steps = 0
    max_steps = max_steps if max_steps is not None else 4 * sample.limit + 4
    while sample.n_out < min(sample.limit, len(sample.out)) and steps < max_steps:
        if redraft is not None:
            redraft(sample)
        base = list(context) + [first] + sample.out[:sample.n_out]
        assert base[-1] == sample.ids[0]
        picks = [pick(base + sample.ids[1:j + 1], sample.draws[j]) for j in range(sample.k + 1)]
        sample.step_end(picks)
        steps += 1
    return steps
