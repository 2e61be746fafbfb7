"""What the tests of s4b_predict_describe share (tests/test_predict_describe.py, tests/test_gpu_predict_describe.py): the numpy model of every output
from a [rows x S] matrix of values, exact — np.sort (-0.0 and +0.0 compare equal and no output tells them apart), one subtraction per width, np.argmin
(the lowest index on a tie), > and < on doubles, the median as xl + 0.5 (xh - xl) (the product by 0.5 is exact, so a contracted multiply-add gives the
same bits) and the MAD likewise — an independent brute force in Python loops, the planted series with their expected values written out, the chains of
tests/test_gpu_predict_groups.py rebuilt, and the device bytes of a call."""
import math
from fractions import Fraction

import numpy as np

import pd_cases as pc
import readout_cases as rc

HDI_MAX, THRESHOLDS_MAX = 8, 32


def median_sorted(xs):
    """Type 7 at 0.5 of rows sorted ascending, [rows x S]: g is 0 (odd S: the middle value itself) or exactly 0.5."""
    S = xs.shape[1]
    lo = (S - 1) // 2
    if S % 2:
        return xs[:, lo].copy()
    return xs[:, lo] + 0.5 * (xs[:, lo + 1] - xs[:, lo])


def model(x, counts=(), thresholds=()):
    """Every output of the call from x [rows x S]: median, mad [rows]; hdi [C x 2 x rows], hdi_start [C x rows]; n_above, n_below [T x rows]."""
    x = np.asarray(x, dtype=np.float64)
    rows, S = x.shape
    xs = np.sort(x, axis=1)
    med = median_sorted(xs)
    mad = median_sorted(np.sort(np.abs(xs - med[:, None]), axis=1))
    hdi, start = np.zeros((len(counts), 2, rows)), np.zeros((len(counts), rows), dtype=np.int32)
    for c, m in enumerate(counts):
        width = xs[:, m - 1:] - xs[:, :S - m + 1]          # [rows x (S - m + 1)]: one subtraction per window
        j = np.argmin(width, axis=1)                        # the lowest index on a tie
        start[c] = j
        hdi[c, 0], hdi[c, 1] = xs[np.arange(rows), j], xs[np.arange(rows), j + m - 1]
    above = np.array([(x > t).sum(axis=1) for t in thresholds], dtype=np.int32).reshape(len(thresholds), rows)
    below = np.array([(x < t).sum(axis=1) for t in thresholds], dtype=np.int32).reshape(len(thresholds), rows)
    return dict(median=med, mad=mad, hdi=hdi, hdi_start=start, n_above=above, n_below=below)


def unique_minimum(x, m):
    """[rows] bool: is the smallest width of the windows of m draws attained by one window only?"""
    xs = np.sort(np.asarray(x, dtype=np.float64), axis=1)
    width = xs[:, m - 1:] - xs[:, :xs.shape[1] - m + 1]
    return (width == width.min(axis=1, keepdims=True)).sum(axis=1) == 1


def brute_force(row, counts=(), thresholds=()):
    """One row in plain Python: sorted(), a loop over every window and every draw."""
    xs = sorted(float(v) for v in row)
    S = len(xs)

    def med(v):
        return v[(S - 1) // 2] if S % 2 else v[S // 2 - 1] + 0.5 * (v[S // 2] - v[S // 2 - 1])
    mid = med(xs)
    out = dict(median=mid, mad=med(sorted(abs(v - mid) for v in xs)), hdi=[], hdi_start=[], n_above=[], n_below=[])
    for m in counts:
        best, at = None, None
        for j in range(S - m + 1):
            w = xs[j + m - 1] - xs[j]
            if best is None or w < best:
                best, at = w, j
        out["hdi"].append((xs[at], xs[at + m - 1]))
        out["hdi_start"].append(at)
    for t in thresholds:
        above = below = 0
        for v in xs:
            above += v > t
            below += v < t
        out["n_above"].append(above)
        out["n_below"].append(below)
    return out


def hdi_draws(ci, S):
    """The m rule of the Python binding restated: ceil(ci x S) in exact rational arithmetic on the decimal text of ci, clamped to [1, S]."""
    return max(1, min(S, math.ceil(Fraction(repr(ci)) * S)))


def midpoint(x):
    """A threshold strictly between two adjacent distinct values of some row of x."""
    for row in np.asarray(x):
        v = np.unique(row)
        if len(v) > 1:
            t = v[0] + 0.5 * (v[1] - v[0])
            if v[0] < t < v[1]:
                return float(t)
    raise AssertionError("no row holds two values with a double between them")


# ---- the planted series (tests/test_gpu_predict_describe.py plants them; tests/test_predict_describe.py holds the model and the brute force against them)
# A group is one call: its pooled draws S, its hdi counts, its thresholds, and name -> (series, expected) with every expected value written out by hand:
# hdi and hdi_start per count, n_above and n_below per threshold.
INF = float("inf")
PLANTED = {
    7: dict(counts=(3, 1, 7, 4), thresholds=(4.0, 1.0, 3.0, 10.0), rows={
        # sorted 0 1 2 4 5 6 9.  m = 3: widths 2 3 3 2 4, windows 0 and 3 tie exactly, the lower wins; m = 4: widths 4 4 4 5.  |x - 4| sorted 0 1 2 2 3 4 5
        "two windows of equal width": ([5.0, 0.0, 9.0, 1.0, 4.0, 2.0, 6.0], dict(
            median=4.0, mad=2.0, hdi=[(0.0, 2.0), (0.0, 0.0), (0.0, 9.0), (0.0, 4.0)], hdi_start=[0, 0, 0, 0], n_above=[3, 5, 4, 0], n_below=[3, 1, 3, 7])),
        # sorted -2 1 1 1 3 7 8.  A draw equal to a threshold counts on neither side: n_above + n_below = S - the ties.  |x - 1| sorted 0 0 0 2 3 6 7
        "draws on a threshold": ([1.0, 7.0, 1.0, -2.0, 3.0, 1.0, 8.0], dict(
            median=1.0, mad=2.0, hdi=[(1.0, 1.0), (-2.0, -2.0), (-2.0, 8.0), (1.0, 3.0)], hdi_start=[1, 0, 0, 1], n_above=[2, 3, 2, 0], n_below=[5, 1, 4, 7])),
        # sorted 0 1 3 3 3 3 4: duplicates straddling the median at odd S.  |x - 3| sorted 0 0 0 0 1 2 3
        "duplicates across the median, odd": ([3.0, 1.0, 3.0, 4.0, 3.0, 3.0, 0.0], dict(
            median=3.0, mad=0.0, hdi=[(3.0, 3.0), (0.0, 0.0), (0.0, 4.0), (3.0, 3.0)], hdi_start=[2, 0, 0, 2], n_above=[0, 5, 1, 0], n_below=[6, 1, 2, 7])),
    }),
    8: dict(counts=(3, 2, 8, 1), thresholds=(0.0, -0.0, 2.0, 2.5, -INF, INF), rows={
        # width 0 everywhere: j = 0
        "all equal": ([2.5] * 8, dict(
            median=2.5, mad=0.0, hdi=[(2.5, 2.5)] * 4, hdi_start=[0, 0, 0, 0], n_above=[8, 8, 8, 0, 8, 0], n_below=[0, 0, 0, 0, 0, 8])),
        # sorted by key -4 -1 -0 -0 +0 +0 2 3: neither zero counts as above or below a threshold of either zero.  |x - 0| sorted 0 0 0 0 1 2 3 4
        "both zeros": ([0.0, -1.0, -0.0, 3.0, -0.0, 2.0, 0.0, -4.0], dict(
            median=0.0, mad=0.5, hdi=[(0.0, 0.0), (0.0, 0.0), (-4.0, 3.0), (-4.0, -4.0)], hdi_start=[2, 2, 0, 0], n_above=[2, 2, 1, 1, 8, 0],
            n_below=[2, 2, 6, 7, 0, 8])),
        # sorted 0 1 2 2 2 2 5 7: duplicates straddling the median at even S, 2 + 0.5 (2 - 2).  |x - 2| sorted 0 0 0 0 1 2 3 5
        "duplicates across the median, even": ([2.0, 5.0, 2.0, 1.0, 2.0, 2.0, 0.0, 7.0], dict(
            median=2.0, mad=0.5, hdi=[(2.0, 2.0), (2.0, 2.0), (0.0, 7.0), (0.0, 0.0)], hdi_start=[2, 2, 0, 0], n_above=[7, 7, 2, 2, 8, 0],
            n_below=[0, 0, 2, 6, 0, 8])),
    }),
}


def assert_planted(got, S, name, i=None):
    """The expected values of planted series `name` of group S against got: a brute_force() result (i None) or a call's outputs at row i."""
    want = PLANTED[S]["rows"][name][1]
    pick = (lambda a: a) if i is None else (lambda a: np.asarray(a)[..., i])
    assert pick(got["median"]) == want["median"] and pick(got["mad"]) == want["mad"], (name, "median, mad")
    hdi = np.asarray(got["hdi"])
    for c, ends in enumerate(want["hdi"]):
        assert tuple(float(v) for v in (hdi[c] if i is None else hdi[c, :, i])) == ends, (name, "hdi", c)
    for k in ("hdi_start", "n_above", "n_below"):
        assert [int(v) for v in (got[k] if i is None else np.asarray(got[k])[:, i])] == want[k], (name, k)


# ---- the chains of tests/test_gpu_predict_groups.py ---------------------------------------------------------------------------------------------------------
class Chain(pc.Chain):
    """pd_cases.Chain with the rows column-major and predict_bart of every stored sampler kept once asked for."""

    def __init__(self, lib, prefix, args, rows, steps):
        super().__init__(lib, prefix, args, steps=steps, rows=rows)
        self._bart = {}
        self.x = np.asfortranarray(self.x)

    def bart(self, S):
        if S not in self._bart:
            self._bart[S] = self.stored[S].predict_bart(self.x)
        return self._bart[S]

    def arm0(self, col):
        """Arm 0's rows: the rows with column `col` overwritten by training values of other rows."""
        x0 = self.x.copy()
        n = len(self.args.x_bart)
        x0[:, col] = self.args.x_bart[(np.arange(len(x0)) * 7 + col + 1) % n, col]
        return x0

    def used_column(self, S):
        return int(np.argmax([self.hit(S, [j]).sum() for j in range(self.P)]))


def gauss_chain(lib, prefix="s4b_"):
    """n = 100, 5 trees; stored samplers of 1, 7, 8, 9, 255, 257 and 2 048 draws."""
    return Chain(lib, prefix, rc._friedman(n=100, T=5, warmup=4, iter=4 + 2048, ranef=False), rows=1100, steps=(1, 6, 1, 1, 246, 2, 1791))


def binary_chain(lib, prefix="s4b_"):
    """n = 400, 11 trees, a binary response; stored samplers of 1, 2, 5 and 13 draws."""
    return Chain(lib, prefix, rc._binary(n=400, T=11, warmup=6, iter=19), rows=300, steps=(1, 1, 3, 8))


def small_chain(lib, prefix):
    """The Gaussian chain cut down to 13 draws (stored samplers of 1, 2, 5 and 13): what the refusals need, on any device layer."""
    return Chain(lib, prefix, rc._friedman(n=100, T=5, warmup=4, iter=4 + 13, ranef=False), rows=60, steps=(1, 1, 3, 8))


def device_bytes_formula(value_bytes, rows, S, Q=0, C=0, T=0, outputs=()):
    """the device memory of one call (every allocation at least 16 bytes) — `value_bytes`: what the value kernel of the arms takes (the
    rows, the trees, the chunk's values 8 C S; quantile_cases' / contrast_cases' formula without per-row outputs, probs and quantiles) — plus the probs
    and one buffer per output asked for, plus the thresholds.  No term grows with rows x S."""
    sizes = []
    if "quantiles" in outputs and Q:
        sizes += [8 * Q, 8 * Q * rows]
    sizes += [8 * rows] * ("median" in outputs) + [8 * rows] * ("mad" in outputs)
    if C:
        sizes += [8 * C * 2 * rows] * ("hdi" in outputs) + [4 * C * rows] * ("hdi_start" in outputs)
    if T:
        sizes += [4 * T * rows] * ("n_above" in outputs) + [4 * T * rows] * ("n_below" in outputs) + [8 * T]
    return value_bytes + sum(max(16, t) for t in sizes)
