"""s4b_predict_groups (stan4bart_amd/csrc/dev_groups.inc over dev_readout.inc, dev_quantile.inc, dev_contrast.inc: k_predict_values / k_contrast_values
unchanged, k_level_reduce, k_level_fold, k_level_rows, k_row_quantiles unchanged) — the model, the bounds and the inputs shared by
tests/test_predict_groups.py (CPU) and tests/test_gpu_predict_groups.py (GPU).

The reference is numpy in long double on the FULL [rows x pooled draws] matrix x, at shapes where it is small: one arm, quantile_cases.model's v
(predict_bart of every pooled sampler plus the linear parts); two arms, contrast_cases.model's d.  With the rows sorted by level (non-decreasing labels)
    a(l, k) = sum_{i : level[i] = l} w_i x(i, k),      A = a (statistic 0) or a / W_l (statistic 1),
W_l the weights of the level added in row order IN DOUBLE, as the host forms it: W_l is part of the definition, not a rounded quantity.

Bound of a(l, k) (u = 2^-53; no measured constant; every comparison allows readout_cases.BOUND_FACTOR x the bound, for the reference's own roundings), in
the style of contrast_cases' `average`.  The device adds the n_l rows of the level in row order within slabs of 64 rows and the slabs' partials in slab
order: on any path at most min(n_l, 64) additions inside a slab and ceil(n_l / 64) between the slabs (a level of n_l rows touches at most
ceil(n_l / 64) + 1 slabs), and one rounding per product:
    bound(a) = sum_i |w_i| bound(x) + (min(n_l, 64) + ceil(n_l / 64) + 1) u sum_i |w_i x|
The division adds one rounding:  bound(A) = bound(a) / W_l + u |A|.
Over the draws: summary_cases.summarise(A, bound(A)) for mean and m2 (k_level_rows forms them as k_contrast_reduce forms a row's: contrast_cases shows
that summarise's bounds hold for that arithmetic, m2 exactly 0 at one draw), quantile_cases.type7 and quantile_cases.bound for the quantiles.
p_above = #{k : A(l, k) > threshold} / S is compared EXACTLY: a pair (l, k) whose reference lies within BOUND_FACTOR x its bound of the threshold
is ambiguous; midway() picks thresholds between two adjacent reference values, so that there is none, and the tests assert that.
A level without rows, or with W_l = 0 under statistic 1: NaN in every floating output on both sides."""
import numpy as np

import quantile_cases as qc
import summary_cases as sc
from readout_cases import BOUND_FACTOR, U, bound_ratio  # noqa: F401

LD = np.longdouble
SLAB = 64          # rows per slab of k_level_reduce (GP_SLAB): part of the interface
LEVEL_BYTES_MAX = 1 << 30          # S4B_GROUPS_LEVEL_BYTES_MAX
FLOATS = ("draws", "mean", "m2", "quantiles")


def level_starts(level, L):
    """The first row of every level of non-decreasing labels, and the end: [L + 1]."""
    level = np.asarray(level)
    assert np.all(np.diff(level) >= 0) and (not len(level) or (level[0] >= 0 and level[-1] < L))
    return np.searchsorted(level, np.arange(L + 1))


def host_weight(w):
    """sum of w in the given order in double: what the host forms."""
    s = 0.0
    for t in np.asarray(w, dtype=np.float64):
        s = s + float(t)
    return s


def model(x, bx, level, L, weights=None, statistic=1, probs=(), threshold=None):
    """`x` [rows x S] (long double or float64) with bounds `bx`, rows sorted by `level`.  Returns (ref, bound): dicts with draws [L x S], mean, m2 [L],
    quantiles [Q x L], p_above [L] (with a threshold), weight, count [L]; ref also `ambiguous`, the number of (level, draw) pairs too close to the
    threshold to be compared."""
    x = np.asarray(x, dtype=LD)
    rows, S = x.shape
    bx = np.broadcast_to(np.asarray(bx, dtype=np.float64), x.shape)
    w = np.ones(rows) if weights is None else np.asarray(weights, dtype=np.float64)
    st = level_starts(level, L)
    A, bA = np.full((L, S), np.nan, dtype=LD), np.full((L, S), np.nan)
    W, count = np.zeros(L), np.diff(st).astype(np.int64)
    for l in range(L):
        i0, i1 = int(st[l]), int(st[l + 1])
        n = i1 - i0
        W[l] = host_weight(w[i0:i1])
        if n == 0 or (statistic == 1 and W[l] == 0.0):
            continue
        wl = w[i0:i1].astype(LD)[:, None]
        a = (wl * x[i0:i1]).sum(axis=0)
        adds = min(n, SLAB) + -(-n // SLAB) + 1
        ba = (np.abs(wl).astype(np.float64) * bx[i0:i1]).sum(axis=0) + adds * U * (np.abs(wl * x[i0:i1])).sum(axis=0).astype(np.float64)
        if statistic == 1:
            A[l] = a / LD(W[l])
            bA[l] = ba / W[l] + U * np.abs(A[l]).astype(np.float64)
        else:
            A[l], bA[l] = a, ba
    ok = ~np.isnan(bA[:, 0])
    ref = dict(draws=A.astype(np.float64), weight=W, count=count, mean=np.full(L, np.nan), m2=np.full(L, np.nan))
    bound = dict(draws=bA, mean=np.full(L, np.nan), m2=np.full(L, np.nan))
    if ok.any():
        r, b = sc.summarise(A[ok], bA[ok])
        for k in ("mean", "m2"):
            ref[k][ok], bound[k][ok] = r[k], b[k]
    if len(probs):
        ref["quantiles"], bound["quantiles"] = np.full((len(probs), L), np.nan), np.full((len(probs), L), np.nan)
        if ok.any():
            ref["quantiles"][:, ok] = qc.type7(A[ok], probs).astype(np.float64)
            bound["quantiles"][:, ok] = qc.bound(A[ok].astype(np.float64), bA[ok], len(probs))
    if threshold is not None:
        t = LD(threshold)
        ref["p_above"] = np.full(L, np.nan)
        ref["p_above"][ok] = (A[ok] > t).sum(axis=1) / float(S)
        near = np.abs(A[ok] - t).astype(np.float64) <= BOUND_FACTOR * bA[ok]
        ref["ambiguous"] = 0 if np.isinf(threshold) else int(near.sum())
    return ref, bound


def midway(A, share=0.5):
    """A threshold midway between two adjacent values of the reference matrix `A` (NaN entries left out): the widest gap among the tenth of the sorted
    values around the quantile `share`."""
    u = np.unique(np.asarray(A, dtype=np.float64)[~np.isnan(np.asarray(A, dtype=np.float64))])
    assert len(u) >= 2, "one distinct value: no gap to put a threshold in"
    c, h = int(share * (len(u) - 1)), max(1, len(u) // 20)
    lo, hi = max(0, c - h), min(len(u) - 1, c + h)
    j = lo + int(np.argmax(np.diff(u[lo:hi + 1])))
    return 0.5 * (u[j] + u[j + 1])


def assert_groups(got, ref, bound, what, report=print):
    """A Sampler.predict_groups result against model(): the same NaN pattern, every finite entry of every floating output within BOUND_FACTOR x its
    bound, weight, count and p_above exactly.  The ratios are printed before they are asserted."""
    ratios = {}
    for key in FLOATS:
        if key in ref and got.get(key) is not None:
            g, r = np.asarray(got[key]), ref[key]
            assert g.shape == r.shape, (what, key, g.shape, r.shape)
            assert np.array_equal(np.isnan(g), np.isnan(r)), f"{what}: {key} has NaN in other places than the model"
            ok = ~np.isnan(r)
            ratios[key] = bound_ratio(g[ok], r[ok], bound[key][ok])
    info = got["info"]
    report(f"predict_groups {what}: route {info['route']}, {info['chunks']} chunk(s) of {info['rows_per_chunk']} rows, {info['edge_levels']} level(s) with edge "
           f"partials, {info['nan_levels']} without an answer; max |device - model| / bound: " + ", ".join(f"{k} {r:.3g}" for k, r in ratios.items()))
    for key, r in ratios.items():
        assert r <= BOUND_FACTOR, f"{what}: {key} is {r:.3g} x the derived bound (allowed: {BOUND_FACTOR:g})"
    if got.get("weight") is not None:
        assert np.array_equal(got["weight"], ref["weight"]), f"{what}: W_l is not the host's sum in row order"
    if got.get("count") is not None:
        assert np.array_equal(got["count"], ref["count"]), f"{what}: count"
    assert info["nan_levels"] == int(np.isnan(ref["mean"]).sum()), (what, info)
    if "p_above" in ref:
        assert ref["ambiguous"] == 0, f"{what}: {ref['ambiguous']} (level, draw) pair(s) lie within their bound of the threshold: choose another threshold"
        assert np.array_equal(got["p_above"], ref["p_above"], equal_nan=True), f"{what}: p_above differs from the model's exact count"
    return ratios


def brute_force(x, level, L, weights=None, statistic=1):
    """Plain numpy, double precision: the group-by loop a user would write over the [rows x draws] matrix."""
    x = np.asarray(x, dtype=np.float64)
    w = np.ones(len(x)) if weights is None else np.asarray(weights, dtype=np.float64)
    out = np.full((L, x.shape[1]), np.nan)
    for l in range(L):
        on = np.asarray(level) == l
        if on.any() and (statistic == 0 or w[on].sum() != 0.0):
            out[l] = (w[on, None] * x[on]).sum(axis=0) / (w[on].sum() if statistic == 1 else 1.0)
    return out


def edge_levels(level, L):
    """The levels that touch more than one slab of 64 rows: what info counts."""
    st = level_starts(level, L)
    return int(sum(1 for l in range(L) if st[l + 1] > st[l] and st[l] // SLAB != (st[l + 1] - 1) // SLAB))


def slab_labels(rows):
    """Non-decreasing labels over `rows` rows that put the reduction's cases next to one another where the rows allow them: a level of one row (row 0), a
    level that ends on row 63 and the next that starts on row 64, a level that is exactly one slab (rows 64 .. 127), a level spanning three slabs and
    more, levels of two rows to the end; an empty level in the middle and one at either end.  Returns (labels, L)."""
    cuts = [0, 1, 64, 128, 128 + 150, 128 + 150 + 700]          # level j + 1 holds rows [cuts[j], cuts[j + 1]); then pairs
    lab = np.zeros(rows, dtype=np.int64)
    nxt = 1                                                      # level 0 stays empty
    for j in range(len(cuts) - 1):
        if cuts[j] >= rows:
            break
        lab[cuts[j]:min(rows, cuts[j + 1])] = nxt
        nxt += 1
        if j == 2:
            nxt += 1                                             # an empty level in the middle
    if rows > cuts[-1]:
        rest = rows - cuts[-1]
        lab[cuts[-1]:] = nxt + np.arange(rest) // 2
        nxt += -(-rest // 2)
    return lab, nxt + 1                                          # (the last level stays empty)


def device_bytes_formula(value_bytes, rows, S, L, C, weights=False, mean=True, m2=True, p_above=False, Q=0, edge=0):
    """the device memory of one call (every allocation at least 16 bytes).  `value_bytes`: what the value kernel's inputs and the
    chunk's scratch take (quantile_cases / contrast_cases.device_bytes_formula without outputs).  No term grows with rows x S beyond the chunk."""
    sizes = [4 * rows, 8 * L * S, 8 * 2 * -(-C // SLAB) * S, 8 * (L + 1), 8 * L, 4 * edge]          # labels, level matrix, edge partials, level starts, W, edge levels
    sizes += [8 * rows] * bool(weights) + [8 * L] * (int(bool(mean)) + int(bool(m2)) + int(bool(p_above)))
    if Q:
        sizes += [8 * Q, 8 * Q * L]
    return value_bytes + sum(max(16, t) for t in sizes)
