"""numpy model of classifier-free guidance for text (include/unimedvl_hip.h, "classifier-free guidance for text").

combine_row is the definition's fp32 chain on bf16 bit patterns, given the two rows' log-sum-exp words: every operation a numpy
float32 operation - one IEEE rounding each, nothing fused - then one round-to-nearest-even to bf16.  lse64 is the fp64 log-sum-exp the
kernel's fp32 words are held against; combine64 the unrounded formula in fp64.  partner() is the header's "active" rule."""
import numpy as np

import penalty_ref as P

NINF = 0xFF80


def lse64(bits):
    """fp64 log-sum-exp of a row of bf16 bit patterns: -inf columns add 0, a NaN makes it NaN, a row of -inf only gives -inf"""
    x = P.bf16_float(bits).astype(np.float64)
    if np.isnan(x).any():
        return np.nan
    m = x.max()
    if m == -np.inf:
        return -np.inf
    return float(m + np.log(np.exp(x - m).sum()))


def row_max(bits):
    """the maximum over the columns that are not NaN (-inf where there is none): exact"""
    x = P.bf16_float(bits)
    x = x[~np.isnan(x)]
    return np.float32(x.max()) if x.size else np.float32(-np.inf)


def floor_of(bits_c, log_beta):
    """the plausibility floor M_c + log_beta as the fp32 word the kernel compares with (log_beta: logf(beta) as an fp32, -inf = off)"""
    with np.errstate(invalid="ignore"):
        return np.float32(row_max(bits_c)) + np.float32(log_beta)


def log_beta(beta):
    """logf(beta) as the host computes it once: an fp32, -inf for beta = 0"""
    return np.float32(-np.inf) if beta == 0 else np.float32(np.log(np.float64(beta)))


def combine_row(bits_c, bits_u, lse_c, lse_u, g, log_beta=-np.inf):
    """uint16 [V] conditional and unconditional rows -> uint16 [V] guided row, by the header's column rule with the fp32 words lse_c /
    lse_u.  A conditional row whose maximum is -inf is returned as it is."""
    if row_max(bits_c) == -np.inf:
        return bits_c.copy()
    lc, lu = P.bf16_float(bits_c).astype(np.float32), P.bf16_float(bits_u).astype(np.float32)
    lse_c, lse_u, g = np.float32(lse_c), np.float32(lse_u), np.float32(g)
    floor = floor_of(bits_c, log_beta)
    with np.errstate(invalid="ignore", over="ignore"):
        cc = (lc - lse_c).astype(np.float32)
        uu = (lu - lse_u).astype(np.float32)
        d = (cc - uu).astype(np.float32)
        a = (g * d).astype(np.float32)
        a = (a + uu).astype(np.float32)
        banned = (lc == -np.inf) | (lc < floor)
    a = np.where(lu == -np.inf, cc, a)
    out = P.bf16_bits(a.astype(np.float32))
    out[banned] = NINF
    return out


def combine64(bits_c, bits_u, g, beta=0.0):
    """float64 [V]: g * (log_softmax(c) - log_softmax(u)) + log_softmax(u) with the edge cases of the definition, unrounded"""
    lc, lu = P.bf16_float(bits_c).astype(np.float64), P.bf16_float(bits_u).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        cc, uu = lc - lse64(bits_c), lu - lse64(bits_u)
        a = g * (cc - uu) + uu
        a = np.where(lu == -np.inf, cc, a)
        banned = lc == -np.inf
        if beta > 0:
            banned |= lc.astype(np.float32) < floor_of(bits_c, log_beta(beta))
    a[banned] = -np.inf
    return a


def kept_by_floor(bits_c, beta):
    """the columns the plausibility floor keeps: l_c >= M_c + logf(beta) in fp32 (beta = 0: every column that is not -inf ... and those)"""
    lc = P.bf16_float(bits_c).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return ~(lc < floor_of(bits_c, log_beta(beta)))


def partner(pair, scale, c, use_scale=True):
    """the unconditional row of row c under the header's rules, -1 where c is not an active guided row"""
    M = len(pair)
    u = int(pair[c])
    if u < 0 or u >= M or u == c:
        return -1
    if use_scale:
        g = float(scale[c])
        if not (np.isfinite(g) and g >= 0) or g == 1.0:
            return -1
    pu = int(pair[u])
    if 0 <= pu < M and pu != u:
        return -1
    if any(int(pair[o]) == u for o in range(c)):
        return -1
    return u


def takes_part(pair, scale):
    """per row: does it take part (active, or the unconditional row of an active row)?"""
    M = len(pair)
    out = [False] * M
    for c in range(M):
        u = partner(pair, scale, c)
        if u >= 0:
            out[c] = out[u] = True
    return out
