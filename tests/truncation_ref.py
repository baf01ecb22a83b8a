"""The tests' fp64 reference of truncated sampling (include/unimedvl_hip.h, "truncated sampling"), on CLASSES - not on a sort of the
columns.  For one row, y[n] = bf16(logit[n] / T); a class is the set of columns that share one value of y (-0 == +0, every NaN is one
class, the highest).  Every filter keeps whole classes at or above a cutoff class:

  top_k: the class that holds the k-th largest value (ties kept), everything when k = 0 or k > V;
  top_p: on what top_k kept (mass Z_k), the first class - descending - at which the cumulative mass reaches top_p Z_k; the mass of a class
         is count * exp(y - M), M the row maximum, the top class count * 1 whatever its value;
  min_p: the lowest class with y - M >= ln(min_p).

The cutoff is the highest of the three.  top_p and min_p are taken at their float32 values, as the device receives them."""
import math
from dataclasses import dataclass

import torch

BF16 = torch.bfloat16


def pick_value(logits, temperature):
    """y of the definition, fp64 [..., V]: bf16(logits / T), the value the sampling keys and the log-probabilities use"""
    return (logits.float() / temperature).to(BF16).double()


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


@dataclass
class Row:
    vals: torch.Tensor      # [C] fp64 class values, descending (a NaN class first)
    cnt: torch.Tensor       # [C] int64 columns per class
    mass: torch.Tensor      # [C] fp64 count * exp(y - M)
    cum: torch.Tensor       # [C] fp64 cumulative mass, descending
    cumcnt: torch.Tensor    # [C] int64 cumulative count
    has_nan: bool

    def index_of(self, value):
        """the class whose value is `value` (float; NaN = the NaN class), None if the row has no such class"""
        if math.isnan(value):
            return 0 if self.has_nan else None
        hit = (self.vals == value).nonzero()
        return int(hit[0]) if hit.numel() else None


def classes(y_row):
    """Row of one row of y (fp64 [V])"""
    y = y_row.clone()
    y[y == 0] = 0.0                                   # -0 == +0
    nan = torch.isnan(y)
    vals, cnt = torch.unique(y[~nan], return_counts=True)
    vals, cnt = vals.flip(0), cnt.flip(0)
    if bool(nan.any()):
        vals = torch.cat([torch.tensor([float("nan")], dtype=torch.float64), vals])
        cnt = torch.cat([nan.sum().reshape(1), cnt])
    w = torch.exp(vals - vals[0])
    w[0] = 1.0                                        # the top class: inf - inf, -inf - -inf and NaN all weigh 1
    mass = cnt.double() * w
    return Row(vals, cnt, mass, mass.cumsum(0), cnt.cumsum(0), bool(nan.any()))


def cutoffs(row, top_k=0, top_p=1.0, min_p=0.0):
    """(ik, ip, im, Zk): the class index of each filter's cutoff (the last class where the filter is off) and the mass top_k kept"""
    last = len(row.vals) - 1
    if row.has_nan:
        return 0, 0, 0, float("nan")
    ik = last
    if top_k > 0 and top_k <= int(row.cumcnt[-1]):
        ik = int((row.cumcnt >= top_k).nonzero()[0])
    zk = float(row.cum[ik])
    ip = last
    if top_p < 1.0:
        ip = int((row.cum >= _f32(top_p) * zk).nonzero()[0])
    im = last
    if min_p > 0.0:
        keep = (row.vals - row.vals[0]) >= math.log(_f32(min_p))
        keep[0] = True
        im = int(keep.nonzero()[-1])
    return ik, ip, im, zk


def cutoff(row, top_k=0, top_p=1.0, min_p=0.0):
    """(class index, cut_y, n_kept) of the definition"""
    ik, ip, im, _ = cutoffs(row, top_k, top_p, min_p)
    i = min(ik, ip, im)
    return i, float(row.vals[i]), int(row.cumcnt[i])


def band(row, top_k=0, top_p=1.0, min_p=0.0, eps=2e-6):
    """(lo, hi): the class indices a device may report as the cutoff.  top_k is exact.  top_p: the mass fraction (of Z_k) at or above
    the class is >= top_p - eps and the fraction strictly above it is < top_p + eps.  min_p: a class with y - M >= ln(min_p) + eps is
    kept, one with y - M <= ln(min_p) - eps is dropped.  The cutoff is the highest of the three, so the interval is the minimum of the
    three intervals' ends."""
    ik, ip, im, zk = cutoffs(row, top_k, top_p, min_p)
    if row.has_nan:
        return 0, 0
    last = len(row.vals) - 1
    plo = phi = mlo = mhi = last
    if top_p < 1.0:
        frac = row.cum / zk if zk > 0 else torch.ones_like(row.cum)
        above = torch.cat([torch.zeros(1, dtype=torch.float64), frac[:-1]])
        ok = ((frac >= _f32(top_p) - eps) & (above < _f32(top_p) + eps)).nonzero()
        plo, phi = int(ok[0]), int(ok[-1])
    if min_p > 0.0:
        d = row.vals - row.vals[0]
        d[0] = 0.0
        ln = math.log(_f32(min_p))
        must = (d >= ln + eps).nonzero()
        mlo = int(must[-1]) if must.numel() else 0
        drop = (d <= ln - eps).nonzero()
        mhi = int(drop[0]) - 1 if drop.numel() else last
        mhi = max(mhi, 0)
    return min(ik, plo, mlo), min(ik, phi, mhi)


def deviation(row, i, top_k=0, top_p=1.0, min_p=0.0):
    """how far into the band class i sits: 0 where it is the definition's own cutoff, else the larger of the mass fraction by which
    it misses top_p and the distance from ln(min_p) of the farthest class sorted against the definition (with several filters on, an
    upper estimate: it does not ask which filter set the cutoff)"""
    exact = cutoff(row, top_k, top_p, min_p)[0]
    if i == exact or row.has_nan:
        return 0.0
    _, _, _, zk = cutoffs(row, top_k, top_p, min_p)
    dev = 0.0
    if top_p < 1.0 and zk > 0:
        at = float(row.cum[i]) / zk
        above = float(row.cum[i - 1]) / zk if i > 0 else 0.0
        dev = max(dev, _f32(top_p) - at, above - _f32(top_p))
    if min_p > 0.0:
        ln = math.log(_f32(min_p))
        lo, hi = min(i, exact), max(i, exact)
        d = (row.vals[lo + 1:hi + 1] - row.vals[0] - ln).abs()          # the classes kept or dropped against the definition
        dev = max(dev, float(d.max()))
    return max(dev, 0.0)


def truncated_probs(row, y_row, i):
    """the renormalised softmax over the columns at or above class i, fp64 [V]"""
    y = y_row.clone()
    keep = torch.isnan(y) if math.isnan(float(row.vals[i])) else (y >= row.vals[i])
    p = torch.where(keep, torch.exp(y - y[keep].max()), torch.zeros_like(y))
    return p / p.sum()
