"""s4b_predict_spread (stan4bart_amd/csrc/readout_spread.inc over dev_readout.inc, dev_quantile.inc, dev_contrast.inc, dev_groups.inc:
k_predict_values / k_contrast_values unchanged, k_spread_reduce, k_spread_fold, k_spread_finish, k_level_rows and k_row_quantiles unchanged) — the
model, the bounds and the inputs shared by tests/test_predict_spread.py (CPU) and tests/test_gpu_predict_spread.py (GPU).

The reference is numpy in long double on the FULL [rows x pooled draws] matrix x, built as group_cases.model takes it: one arm, quantile_cases.model's
v; two arms, contrast_cases.model's d.  With weights w_i >= 0, W = the weights added in row order IN DOUBLE (group_cases.host_weight: part of the
definition) and ascending thresholds t_j, per draw k
    mean = w' x / W,   M2 = sum_i w_i (x_i - mean)^2,   sd = sqrt(M2 / W),   min, max over the rows with w_i > 0,
    share_above[j] = (sum of w_i over x_i > t_j) / W,   part_above[j] = (sum of w_i x_i over x_i > t_j) / W,
the matrix D [(4 + 2 T) x S] in that order, and over the draws summary_cases.summarise (mean, m2: k_level_rows' arithmetic, as group_cases uses it),
quantile_cases.type7 and quantile_cases.bound.

BOUNDS (u = 2^-53; no measured constant; every comparison allows readout_cases.BOUND_FACTOR x the bound, for the reference's own roundings and the
terms of second order).  bx is the bound of x.  Per draw let
    B = SLAB,  slabs = ceil(n / B),  adds = min(n, B) + slabs + 1   (the additions a term passes inside its slab and between the slabs, plus one),
    rng = max_i x_i - min_i x_i + 2 max_i bx_i   over ALL rows (the shift c of a slab is its first row's value, whatever that row's weight),
    amax = max_i |x_i| + max_i bx_i.
Every difference the device forms — x - c, mean_b - mean_a — is at most rng in magnitude, every value at most amax.
Weights.  W_s and the running W_a are left folds of non-negative terms: relative error at most adds u.
Slab means.  s1 = fold of w (x - c): a subtraction, a product and at most min(n, B) additions per term, |s1 error| <= (adds + 2) u W_s rng;
s1 / W_s adds the error of W_s and a division: |error of mean_s - c| <= (2 adds + 3) u rng; c + s1 / W_s adds u amax.
Pairwise update.  mean' = mean_a + delta W_b / W is a convex combination of mean_a and mean_b, so the errors of its inputs do not grow; the step
itself rounds delta (u rng), the product, the sum W and the division (each relative u, W_b and W each carrying adds u):
at most (2 adds + 5) u rng (W_b / W) + u amax.  Over at most slabs - 1 steps, W_b / W <= 1:
    bound(mean) = w' bx / W + cnt u rng + (slabs + 1) u amax,          cnt = slabs (2 adds + 5).
Second moment.  Every term of M2 is a weight times the product of two differences, so M2 <= W rng^2.  In a slab s2 carries (adds + 3) u W_s rng^2,
s1^2 / W_s (3 adds + 6) u W_s rng^2 and the subtraction u W_s rng^2; over the slabs (4 adds + 10) u W rng^2.  A step adds delta^2 W_a W_b / W
<= rng^2 W_b: delta carries the rounding part of two means, 2 (cnt u rng + (slabs + 1) u amax) + u rng, so delta^2 carries
2 rng ((2 cnt + 1) u rng + 2 (slabs + 1) u amax); the weights 3 adds + 4 roundings; the two additions of a step 2 u W rng^2.  Summed (sum of W_b <= W):
    rounding(M2) = ((4 cnt + 7 adds + 2 slabs + 16) rng^2 + 4 (slabs + 1) amax rng) u W
and the inputs move M2 by at most sum_i w_i (2 |x_i - mean| e_i + e_i^2), e_i = bx_i + w' bx / W:
    bound(M2) = sum_i w_i (2 |x_i - mean| e_i + e_i^2) + rounding(M2).
The term amax rng u W is what the shift buys: raw moments would carry amax^2 u W.
sd = sqrt(M2 / W): with bV = bound(M2) / W + u M2 / W and |sqrt a - sqrt b| <= min(sqrt |a - b|, |a - b| / sqrt b):
    bound(sd) = min(sqrt(bV), bV / sd) + 2 u sd.
Extremes.  bound(min) = bound(max) = max_i bx_i.
Bins.  A value within BOUND_FACTOR x bx of a finite threshold is AMBIGUOUS: the device may put it in another bin.  The cases take their finite
thresholds from group_cases.midway over the reference matrix, `ambiguous` counts every (row, draw, threshold) triple and the tests assert that there
is none; then the device and the model add the same rows.  cw, cs pass at most min(n, B) additions in a slab, slabs between them, T in the suffix
sum and a division; the terms of share are non-negative:
    bound(share_above) = 0 without weights (counts: exact in double; compared EXACTLY), else (adds + T + 1) u share_above
    bound(part_above)  = (sum over the rows above of w_i bx_i) / W + (adds + T + 2) u (sum over the rows above of w_i |x_i|) / W.

DEVICE MEMORY of one call (device_bytes_formula): the value kernel's inputs and the chunk's scratch 8 C S, and beyond them, with
R = 5 + 2 (T + 1) and M = 4 + 2 T: the weights 8 n (if given), the thresholds 8 T, the slab partials 8 ceil(C / SLAB) R S, the totals 8 R S, the matrix
8 M S, the M + 1 row marks, M unit weights, M doubles per summary asked for, the probs and 8 Q M.  Nothing grows with n x S beyond the chunk."""
import numpy as np

import group_cases as gc
import quantile_cases as qc
import summary_cases as sc
from readout_cases import BOUND_FACTOR, U, bound_ratio  # noqa: F401

LD = np.longdouble
SLAB = 128              # rows per slab of k_spread_reduce (SP_SLAB, S4B_SPREAD_SLAB): part of the interface
THRESHOLDS_MAX = 64     # S4B_SPREAD_THRESHOLDS_MAX
FLOATS = ("draws", "mean", "m2", "quantiles")


def names(T):
    return ["mean", "sd", "min", "max"] + [f"share_above[{j}]" for j in range(T)] + [f"part_above[{j}]" for j in range(T)]


def model(x, bx, weights=None, thresholds=(), probs=()):
    """`x` [rows x S] (long double or float64) with bounds `bx`.  Returns (ref, bound): dicts with draws [(4 + 2 T) x S], mean, m2 [4 + 2 T],
    quantiles [Q x (4 + 2 T)]; ref also weight, zero_slabs and `ambiguous`, the number of (row, draw, threshold) triples too close to a finite
    threshold to be binned alike on both sides."""
    x = np.asarray(x, dtype=LD)
    n, S = x.shape
    bx = np.broadcast_to(np.asarray(bx, dtype=np.float64), x.shape)
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    th = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    T = len(th)
    assert np.all(np.diff(th) > 0) and not np.any(np.isnan(th))
    W = gc.host_weight(w)
    assert W > 0.0, "the call is refused: no weight"
    wl = w.astype(LD)[:, None]
    on = w > 0.0
    slabs = -(-n // SLAB)
    adds = min(n, SLAB) + slabs + 1
    cnt = slabs * (2 * adds + 5)
    xf = x.astype(np.float64)
    bmax = bx.max(axis=0)
    rng = (xf.max(axis=0) - xf.min(axis=0)) + 2.0 * bmax
    amax = np.abs(xf).max(axis=0) + bmax
    mean = (wl * x).sum(axis=0) / LD(W)
    dev = x - mean[None, :]
    M2 = (wl * dev * dev).sum(axis=0)
    sd = np.sqrt(M2 / LD(W))
    wbx = (w[:, None] * bx).sum(axis=0) / W
    bmean = wbx + cnt * U * rng + (slabs + 1) * U * amax
    e = bx + wbx[None, :]
    bM2 = (w[:, None] * (2.0 * np.abs(dev).astype(np.float64) * e + e * e)).sum(axis=0) \
        + ((4 * cnt + 7 * adds + 2 * slabs + 16) * rng * rng + 4.0 * (slabs + 1) * amax * rng) * U * W
    bV = bM2 / W + U * (M2 / LD(W)).astype(np.float64)
    sdf = sd.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        bsd = np.where(sdf > 0.0, np.minimum(np.sqrt(bV), bV / np.where(sdf > 0.0, sdf, 1.0)), np.sqrt(bV)) + 2.0 * U * sdf
    D = np.zeros((4 + 2 * T, S), dtype=LD)
    bD = np.zeros((4 + 2 * T, S))
    D[0], D[1], D[2], D[3] = mean, sd, x[on].min(axis=0), x[on].max(axis=0)
    bD[0], bD[1], bD[2], bD[3] = bmean, bsd, bmax, bmax
    ambiguous = 0
    for j, t in enumerate(th):
        above = x > LD(t)
        D[4 + j] = (wl * above).sum(axis=0) / LD(W)
        if weights is None:          # counts: the double quotient count / n itself, which is what "exactly" means
            D[4 + j] = above.sum(axis=0).astype(np.float64) / W
        D[4 + T + j] = (wl * np.where(above, x, LD(0))).sum(axis=0) / LD(W)
        bD[4 + j] = 0.0 if weights is None else (adds + T + 1) * U * D[4 + j].astype(np.float64)
        bD[4 + T + j] = (w[:, None] * np.where(above, bx, 0.0)).sum(axis=0) / W \
            + (adds + T + 2) * U * (w[:, None] * np.where(above, np.abs(xf), 0.0)).sum(axis=0) / W
        if np.isfinite(t):
            ambiguous += int((np.abs(x - LD(t)).astype(np.float64) <= BOUND_FACTOR * bx).sum())
    zero_slabs = int(sum(1 for s in range(slabs) if gc.host_weight(w[s * SLAB:(s + 1) * SLAB]) == 0.0))
    ref = dict(draws=D, weight=W, zero_slabs=zero_slabs, ambiguous=ambiguous, thresholds=th)
    bound = dict(draws=bD)
    r, b = sc.summarise(D, bD)
    ref["mean"], ref["m2"], bound["mean"], bound["m2"] = r["mean"], r["m2"], b["mean"], b["m2"]
    if len(probs):
        ref["quantiles"] = qc.type7(D, probs).astype(np.float64)
        bound["quantiles"] = qc.bound(D.astype(np.float64), bD, len(probs))
    return ref, bound


def device_order(x, weights=None, thresholds=()):
    """The statement of include/stan4bart_amd.h carried out literally in double, one draw at a time: slabs of SLAB rows, the shift, the left folds,
    the pairwise update in slab order, the bins, the suffix sums.  Without fused multiply-adds, so it agrees with a device to rounding only; the CPU
    tests hold it against model() within the bounds, which checks that the bounds cover the stated order."""
    x = np.asarray(x, dtype=np.float64)
    n, S = x.shape
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    th = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    T = len(th)
    W = gc.host_weight(w)
    D = np.zeros((4 + 2 * T, S))
    for k in range(S):
        Wa = mean = M2 = 0.0
        mn, mx = np.inf, -np.inf
        cw, cs = np.zeros(T + 1), np.zeros(T + 1)
        for r0 in range(0, n, SLAB):
            xs, ws = x[r0:r0 + SLAB, k], w[r0:r0 + SLAB]
            c, Ws, s1, s2 = xs[0], 0.0, 0.0, 0.0
            pw, ps = np.zeros(T + 1), np.zeros(T + 1)
            for xi, wi in zip(xs, ws):
                d = xi - c
                Ws, s1, s2 = Ws + wi, s1 + wi * d, s2 + (wi * d) * d
                if wi > 0.0:
                    mn, mx = min(mn, xi), max(mx, xi)
                b = int((xi > th).sum())
                pw[b] += wi
                ps[b] += wi * xi
            cw, cs = cw + pw, cs + ps
            if not Ws > 0.0:
                continue
            ms, Ms = c + s1 / Ws, max(0.0, s2 - s1 * s1 / Ws)
            if not Wa > 0.0:
                Wa, mean, M2 = Ws, ms, Ms
                continue
            delta, Wn = ms - mean, Wa + Ws
            mean, M2, Wa = mean + delta * Ws / Wn, M2 + Ms + delta * delta * Wa * Ws / Wn, Wn
        D[0, k], D[1, k], D[2, k], D[3, k] = mean, np.sqrt(M2 / W), mn, mx
        aw = as_ = 0.0
        for b in range(T, 0, -1):
            aw, as_ = aw + cw[b], as_ + cs[b]
            D[4 + b - 1, k], D[4 + T + b - 1, k] = aw / W, as_ / W
    return D


def brute_force(x, weights=None, thresholds=()):
    """Plain numpy, double precision: what a user would write over the [rows x draws] matrix."""
    x = np.asarray(x, dtype=np.float64)
    n, S = x.shape
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    T = len(thresholds)
    D = np.zeros((4 + 2 * T, S))
    for k in range(S):
        D[0, k] = np.average(x[:, k], weights=w)
        D[1, k] = np.sqrt(np.cov(x[:, k], aweights=w, ddof=0)) if n > 1 else 0.0
        D[2, k], D[3, k] = x[w > 0.0, k].min(), x[w > 0.0, k].max()
        for j, t in enumerate(thresholds):
            D[4 + j, k] = w[x[:, k] > t].sum() / w.sum()
            D[4 + T + j, k] = (w * x[:, k])[x[:, k] > t].sum() / w.sum()
    return D


def thresholds_for(x, T, lo_inf=False, hi_inf=False):
    """T strictly ascending thresholds for the reference matrix `x`: -inf first and +inf last where asked for, the finite ones from
    group_cases.midway over consecutive blocks of the sorted distinct values (so that they differ and ascend), each midway between two adjacent
    reference values."""
    n_fin = T - int(lo_inf) - int(hi_inf)
    assert n_fin >= 0
    u = np.unique(np.asarray(x, dtype=np.float64))
    assert len(u) >= 2 * n_fin, f"{len(u)} distinct values do not hold {n_fin} thresholds"
    edges = np.linspace(0, len(u), n_fin + 1).astype(int)
    fin = [gc.midway(u[edges[j]:edges[j + 1]]) for j in range(n_fin)]
    th = np.array(([-np.inf] if lo_inf else []) + fin + ([np.inf] if hi_inf else []), dtype=np.float64)
    assert len(th) == T and np.all(np.diff(th) > 0)
    return th


def assert_spread(got, ref, bound, what, report=print, weighted=False):
    """A Sampler.predict_spread result against model(): every floating output within BOUND_FACTOR x its bound, none left out; W exactly; without
    weights share_above exactly (its bound is 0).  The ratios are printed before they are asserted."""
    info = got["info"]
    T = len(ref["thresholds"])
    assert ref["ambiguous"] == 0, f"{what}: {ref['ambiguous']} (row, draw, threshold) triple(s) lie within their bound of a threshold: choose other thresholds"
    assert got["weight"] == ref["weight"], f"{what}: W is not the host's sum in row order"
    assert info["thresholds"] == T and info["zero_slabs"] == ref["zero_slabs"], (what, info, ref["zero_slabs"])
    ratios = {}
    for key in FLOATS:
        if key in ref and got.get(key) is not None:
            g, r = np.asarray(got[key]), np.asarray(ref[key])
            assert g.shape == r.shape, (what, key, g.shape, r.shape)
            assert np.all(np.isfinite(g)), f"{what}: {key} holds a value that is not finite"
            ratios[key] = bound_ratio(g, r, bound[key])
    g, r, b = np.asarray(got["draws"]), ref["draws"], bound["draws"]
    parts = {"d.mean": slice(0, 1), "d.sd": slice(1, 2), "d.minmax": slice(2, 4)}
    if T:
        parts.update({"d.share": slice(4, 4 + T), "d.part": slice(4 + T, 4 + 2 * T)})
    for key, rows in parts.items():
        ratios[key] = bound_ratio(g[rows], r[rows], b[rows])
    report(f"predict_spread {what}: route {info['route']}, {info['chunks']} chunk(s) of {info['rows_per_chunk']} rows, T = {T}, {info['draws']} draws, "
           f"{info['zero_slabs']} slab(s) without weight; max |device - model| / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    for key, v in ratios.items():
        assert v <= BOUND_FACTOR, f"{what}: {key} is {v:.3g} x the derived bound (allowed: {BOUND_FACTOR:g})"
    if T and not weighted:
        assert np.array_equal(g[4:4 + T], r[4:4 + T].astype(np.float64)), f"{what}: share_above differs from the model's exact count / n"
    return ratios


def device_bytes_formula(value_bytes, rows, S, T, C, weights=False, mean=True, m2=True, Q=0):
    """the device memory of one call (every allocation at least 16 bytes).  `value_bytes`: what the value kernel's inputs and the
    chunk's scratch take (quantile_cases / contrast_cases.device_bytes_formula without outputs).  No term grows with rows x S beyond the chunk."""
    R, M = 5 + 2 * (T + 1), 4 + 2 * T
    sizes = [8 * -(-C // SLAB) * R * S, 8 * R * S, 8 * M * S, 8 * (M + 1), 8 * M]
    sizes += [8 * rows] * bool(weights) + [8 * T] * bool(T) + [8 * M] * (int(bool(mean)) + int(bool(m2)))
    if Q:
        sizes += [8 * Q, 8 * Q * M]
    return value_bytes + sum(max(16, t) for t in sizes)
