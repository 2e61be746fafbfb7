"""What the tests of s4b_predict_sorted share (tests/test_predict_sorted.py, tests/test_gpu_predict_sorted.py): the numpy model of every output from a
[rows x S] matrix of values — the monotone key of a double in uint64 (negative: all bits flipped, else the sign bit set; -0.0 before +0.0), a sort of
the keys per column, the ranks, R's type 7 ACROSS THE ROWS with h, lo, hi and g formed in double as the host forms them, and the strict counts in
double comparison — an independent brute force in Python loops (sorted() with the key), the planted matrices with their expected values written out
where small, and the top / bottom rule of the Python binding."""
import math
import struct
from fractions import Fraction

import numpy as np

PROBS_MAX, CUTS_MAX, TARGETS_MAX, DRAWS_PER_BLOCK_MAX, PASSES = 12, 8, 32, 1024, 8


def key(x):
    """qt_key: the order-preserving map of a double's bits to uint64."""
    b = np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def value(k):
    """qt_value: the inverse of key()."""
    k = np.asarray(k, dtype=np.uint64)
    return np.where(k >> np.uint64(63), k & np.uint64((1 << 63) - 1), ~k).astype(np.uint64).view(np.float64)


def sorted_columns(x):
    """Every column of x [rows x S] in key order: [rows x S] float64, the bits of the values kept (-0.0 before +0.0)."""
    return value(np.sort(key(x), axis=0))


def type7_rows(p, n):
    """(lo, hi, g) of R's type 7 across n rows at prob p, in double as qt_type7_rows forms them."""
    h = float(p) * float(n - 1)
    lo = min(int(math.floor(h)), n - 1)
    return lo, min(lo + 1, n - 1), h - float(lo)


def model(x, row_probs=(), cut_rank=()):
    """sorted [Qr x S] (xl + g (xh - xl) in double, uncontracted; xl itself where g = 0), its bracket lo, hi [Qr x S] and g [Qr]; cut [J x S];
    n_above, n_below [J x rows] int32."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    n, S = x.shape
    y = sorted_columns(x)
    Qr, J = len(row_probs), len(cut_rank)
    srt, lo_v, hi_v, gs = np.zeros((Qr, S)), np.zeros((Qr, S)), np.zeros((Qr, S)), np.zeros(Qr)
    for j, p in enumerate(row_probs):
        lo, hi, g = type7_rows(p, n)
        lo_v[j], hi_v[j], gs[j] = y[lo], y[hi], g
        srt[j] = y[lo] if g == 0.0 else y[lo] + g * (y[hi] - y[lo])
    cut = np.array([y[r] for r in cut_rank], dtype=np.float64).reshape(J, S)
    above = np.array([(x > cut[c][None, :]).sum(axis=1) for c in range(J)], dtype=np.int32).reshape(J, n)
    below = np.array([(x < cut[c][None, :]).sum(axis=1) for c in range(J)], dtype=np.int32).reshape(J, n)
    return dict(sorted=srt, lo=lo_v, hi=hi_v, g=gs, cut=cut, n_above=above, n_below=below)


def _py_key(v):
    b = struct.unpack("<Q", struct.pack("<d", v))[0]
    return (~b) & ((1 << 64) - 1) if b >> 63 else b | (1 << 63)


def brute_force(x, row_probs=(), cut_rank=()):
    """The same outputs in plain Python: sorted() with the key per column, loops over every row and draw."""
    rows = [[float(v) for v in r] for r in np.asarray(x, dtype=np.float64)]
    n, S = len(rows), len(rows[0])
    cols = [sorted((rows[i][k] for i in range(n)), key=_py_key) for k in range(S)]
    out = dict(sorted=[], cut=[], n_above=[], n_below=[])
    for p in row_probs:
        h = p * (n - 1)
        lo = min(int(h // 1), n - 1)
        hi, g = min(lo + 1, n - 1), h - lo
        out["sorted"].append([c[lo] if g == 0.0 else c[lo] + g * (c[hi] - c[lo]) for c in cols])
    for r in cut_rank:
        cut = [c[r] for c in cols]
        out["cut"].append(cut)
        out["n_above"].append([sum(1 for k in range(S) if rows[i][k] > cut[k]) for i in range(n)])
        out["n_below"].append([sum(1 for k in range(S) if rows[i][k] < cut[k]) for i in range(n)])
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def fraction_count(f, n):
    """The m rule of the Python binding restated: ceil(f x n) in exact rational arithmetic on the decimal text of f."""
    return math.ceil(Fraction(repr(float(f))) * n)


def group_ranks(n, top=(), bottom=()):
    """The cut ranks of the binding: top fraction f -> n - m - 1 (the m rows strictly above it), bottom -> m (the m rows strictly below it)."""
    return [n - fraction_count(f, n) - 1 for f in top] + [fraction_count(f, n) for f in bottom]


def blocks(S, Db):
    """The blocks of draws of a call: [(first draw, draws)]."""
    return [(k, min(Db, S - k)) for k in range(0, S, Db)]


def draws_per_block(n, S, scratch_bytes=0, default=64 << 20):
    """The draws of a block as the library chooses them: whole groups of 8 that the scratch holds, 8 at least, 1024 at most; all draws where they fit."""
    scratch = min(scratch_bytes, default) if scratch_bytes > 0 else default
    Db = min(DRAWS_PER_BLOCK_MAX, max(8, scratch // (8 * n) // 8 * 8))
    return S if Db >= S else Db


def targets(n, row_probs=(), cut_rank=()):
    """The distinct ranks a call selects per draw: lo (and hi where g > 0) of every row prob, and the cut ranks."""
    t = set(int(r) for r in cut_rank)
    for p in row_probs:
        lo, hi, g = type7_rows(p, n)
        t.add(lo)
        if g != 0.0:
            t.add(hi)
    return sorted(t)


def launches(S, Db, counts, summary):
    """Kernel launches of a call: per block the value kernel, 8 x (hist, scan) and the counts; the finish; the summary's."""
    return len(blocks(S, Db)) * (1 + 2 * PASSES + (1 if counts else 0)) + 1 + summary


# ---- planted matrices, small, with their expected values written out -------------------------------------------------------------------------------------------
NZ = -0.0
PLANTED = {
    # one draw, five rows: sorted by key -1 -0 -0 +0 2.  Rank 1 and 2 are -0.0, rank 3 is +0.0: the sign follows the key order.  Against a zero cut the
    # zeros count on neither side.
    "both zeros": dict(x=[[0.0], [NZ], [2.0], [NZ], [-1.0]], ranks=(0, 1, 2, 3, 4), order_stats=[[-1.0], [NZ], [NZ], [0.0], [2.0]], cut_rank=(1, 3, 4, 0),
                       n_above=[[0, 0, 1, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 0]],
                       n_below=[[0, 0, 0, 0, 1], [0, 0, 0, 0, 1], [1, 1, 0, 1, 1], [0, 0, 0, 0, 0]]),
    # two draws, four rows: column 0 is 3 1 1 2 (sorted 1 1 2 3), column 1 is 5 5 5 5
    "ties and a constant column": dict(x=[[3.0, 5.0], [1.0, 5.0], [1.0, 5.0], [2.0, 5.0]], ranks=(3, 0, 1, 2, 1),
                                       order_stats=[[3.0, 5.0], [1.0, 5.0], [1.0, 5.0], [2.0, 5.0], [1.0, 5.0]], cut_rank=(1, 2),
                                       n_above=[[1, 0, 0, 1], [1, 0, 0, 0]], n_below=[[0, 0, 0, 0], [0, 1, 1, 0]]),
    # one row: every rank is 0
    "one row": dict(x=[[7.5, -2.0, 0.0]], ranks=(0, 0), order_stats=[[7.5, -2.0, 0.0]] * 2, cut_rank=(0,), n_above=[[0]], n_below=[[0]]),
}
