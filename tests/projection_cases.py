"""s4b_predict_projection (stan4bart_amd/csrc/readout_projection.inc over dev_readout.inc, dev_quantile.inc, dev_contrast.inc, dev_groups.inc:
k_predict_values / k_contrast_values unchanged, k_proj_reduce, k_proj_fold, k_proj_solve, k_level_rows and k_row_quantiles unchanged) — the model, the
bounds and the inputs shared by tests/test_predict_projection.py (CPU) and tests/test_gpu_predict_projection.py (GPU).

The reference is numpy in long double on the FULL [rows x pooled draws] matrix x, built as group_cases.model takes it: one arm, quantile_cases.model's
v; two arms, contrast_cases.model's d.  With the design A [n x K] and weights w_i >= 0
    G = A' W A,   b = A' W x,   s = w' x,   t = w' x^2,   W = the weights added in row order IN DOUBLE (group_cases.host_weight: part of the definition),
    G = L L' (long-double Cholesky),   beta = G^-1 b,   rss = t - sum_j beta_j b_j,   tss = t - s^2 / W,   r2 = 1 - rss / tss (NaN where tss == 0).
The design is deficient where a pivot d_j <= tol G(j,j); then, with n = 0 and with W = 0, every floating output is NaN on both sides.

BOUNDS (u = 2^-53; no measured constant; every comparison allows readout_cases.BOUND_FACTOR x the bound, for the reference's own roundings and the
terms of second order).
Moments.  The device adds the n rows in row order within slabs of B = SLAB rows and the slabs' partials in slab order: a term passes at most
min(n, B) - 1 additions inside its slab and ceil(n / B) - 1 between the slabs, and is itself the rounded product of at most three factors (w x, then
times A(i,j) or x; a fused multiply-add only removes a rounding): at most min(n, B) + ceil(n / B) roundings, one fewer than the count
    adds = min(n, B) + ceil(n / B) + 1
that the bounds take.  With |.| entrywise and bx the bound of x:
    bound(b) = |W A|' bx + adds u |W A|' |x|           bound(G) = adds u |A|' |W A|   (no input error)
    bound(s) = w' bx + adds u w' |x|                   bound(t) = w' (2 |x| bx + bx^2) + adds u w' x^2
Coefficients.  The device solves (G^ + dG) beta^ = b^ with G^ = G + eG, |eG| <= bound(G), b^ = b + eb, |eb| <= bound(b), and dG the backward error of
the Cholesky solve: |dG| <= gamma_{3K+1} |L^| |L^'|, gamma_m = m u / (1 - m u) (N. J. Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.,
SIAM 2002, Theorem 10.4).  To first order, componentwise (ibid., section 7.2):
    bound(beta) = |G^-1| (bound(b) + (bound(G) + gamma_{3K+1} |L| |L'|) |beta|)
rss, tss and r2 term by term (K products and K subtractions; a product, a division and a subtraction; a division and a subtraction):
    bound(rss) = bound(t) + sum_j (|beta_j| bound(b_j) + |b_j| bound(beta_j)) + (K + 1) u (|t| + sum_j |beta_j b_j|)
    bound(tss) = bound(t) + 2 |s| bound(s) / W + 3 u (|t| + s^2 / W)
    bound(r2)  = bound(rss) / |tss| + |rss| bound(tss) / tss^2 + 3 u (1 + |rss / tss|)
Over the draws: summary_cases.summarise for mean and m2 (k_level_rows' arithmetic, as group_cases uses it), quantile_cases.type7 and
quantile_cases.bound for the quantiles.  p_above is compared EXACTLY; group_cases.midway picks a threshold between two adjacent reference values and
`ambiguous` counts the (row, draw) pairs within BOUND_FACTOR x their bound of it: the tests assert that there is none.

The test designs are well conditioned — standard normal columns beside an intercept — and check_inputs asserts it: cond(G) <= 1e4 and the largest
bound of r2 <= 1e-6, so that a comparison within the bound means something.

DEVICE MEMORY of one call (device_bytes_formula): the value kernel's inputs and the chunk's scratch 8 C S, and beyond them, with
KT = K rounded up to 8, 16 or 32: the padded design 8 n KT, the weights 8 n (if given), the slab partials 8 ceil(C / SLAB) (K + 2) max(S, K), the
totals 8 (K + 2) K and 8 (K + 2) S, the matrix 8 (K + 1) S, the K + 2 row marks and the flag, K + 1 unit weights, K + 1 doubles per summary asked
for, the probs and 8 Q (K + 1).  Nothing grows with n x S beyond the chunk."""
import numpy as np

import group_cases as gc
import quantile_cases as qc
import summary_cases as sc
from readout_cases import BOUND_FACTOR, U, bound_ratio  # noqa: F401

LD = np.longdouble
SLAB = 128          # rows per slab of k_proj_reduce (PJ_SLAB, S4B_PROJECTION_SLAB): part of the interface
COLUMNS_MAX = 32    # S4B_PROJECTION_COLUMNS_MAX
TOL = 1e-10
FLOATS = ("coef", "r2", "mean", "m2", "quantiles")


def gamma(m):
    return m * U / (1.0 - m * U)


def cholesky(G, tol=TOL):
    """Lower factor of G in long double, column by column as the device forms it; (L, deficient)."""
    G = np.asarray(G, dtype=LD)
    K = len(G)
    L = np.zeros((K, K), dtype=LD)
    for j in range(K):
        d = G[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not d > LD(tol) * G[j, j]:
            return L, True
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, K):
            L[i, j] = (G[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L, False


def chol_solve(L, B):
    """G^-1 B by the two substitutions, long double."""
    K = len(L)
    Y = np.array(B, dtype=LD, copy=True)
    for j in range(K):
        Y[j] = (Y[j] - (L[j, :j, None] * Y[:j]).sum(axis=0)) / L[j, j]
    for j in range(K - 1, -1, -1):
        Y[j] = (Y[j] - (L[j + 1:, j, None] * Y[j + 1:]).sum(axis=0)) / L[j, j]
    return Y


def model(x, bx, design, weights=None, probs=(), threshold=None, tol=TOL):
    """`x` [rows x S] (long double or float64) with bounds `bx`, `design` [rows x K].  Returns (ref, bound): dicts with coef [K x S], r2 [S], mean, m2
    [K + 1], quantiles [Q x (K + 1)], p_above [K + 1] (with a threshold); ref also weight, deficient (0, 1 deficient design, 2 W == 0, 3 no rows),
    moments (G, b, s, t with their bounds, for the tests of the model itself) and `ambiguous`."""
    x = np.asarray(x, dtype=LD)
    n, S = x.shape
    A = np.asarray(design, dtype=np.float64)
    A = A[:, None] if A.ndim == 1 else A
    assert A.ndim == 2 and A.shape[0] == n, (A.shape, n)
    K = A.shape[1]
    bx = np.broadcast_to(np.asarray(bx, dtype=np.float64), x.shape)
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    W = gc.host_weight(w)
    Q = len(probs)
    nanref = dict(coef=np.full((K, S), np.nan), r2=np.full(S, np.nan), mean=np.full(K + 1, np.nan), m2=np.full(K + 1, np.nan), weight=W, ambiguous=0)
    if Q:
        nanref["quantiles"] = np.full((Q, K + 1), np.nan)
    if threshold is not None:
        nanref["p_above"] = np.full(K + 1, np.nan)
    if n == 0 or W == 0.0:
        return dict(nanref, deficient=3 if n == 0 else 2), {}
    Al, wl = A.astype(LD), w.astype(LD)
    WA = wl[:, None] * Al
    G, b, s, t = Al.T @ WA, WA.T @ x, wl @ x, wl @ (x * x)
    adds = min(n, SLAB) + -(-n // SLAB) + 1
    aWA, ax = np.abs(WA).astype(np.float64), np.abs(x).astype(np.float64)
    bG = adds * U * (np.abs(A).T @ aWA)
    bb = aWA.T @ bx + adds * U * (aWA.T @ ax)
    bs = w @ bx + adds * U * (w @ ax)
    bt = w @ (2.0 * ax * bx + bx * bx) + adds * U * (w @ (ax * ax))
    moments = dict(G=G, b=b, s=s, t=t, bG=bG, bb=bb, bs=bs, bt=bt)
    L, deficient = cholesky(G, tol)
    if deficient:
        return dict(nanref, deficient=1, moments=moments), {}
    beta = chol_solve(L, b)
    Ginv = np.abs(chol_solve(L, np.eye(K, dtype=LD))).astype(np.float64)
    LL = (np.abs(L) @ np.abs(L).T).astype(np.float64)
    ab, abeta = np.abs(b).astype(np.float64), np.abs(beta).astype(np.float64)
    bbeta = Ginv @ (bb + (bG + gamma(3 * K + 1) * LL) @ abeta)
    fit = (beta * b).sum(axis=0)
    rss, tss = t - fit, t - s * s / LD(W)
    at, s2W = np.abs(t).astype(np.float64), (s * s / LD(W)).astype(np.float64)
    brss = bt + (abeta * bb + ab * bbeta).sum(axis=0) + (K + 1) * U * (at + (abeta * ab).sum(axis=0))
    btss = bt + 2.0 * np.abs(s).astype(np.float64) * bs / W + 3.0 * U * (at + s2W)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = rss / tss
        r2 = np.where(tss == 0, LD(np.nan), 1 - ratio)
        atss = np.abs(tss).astype(np.float64)
        br2 = brss / atss + np.abs(rss).astype(np.float64) * btss / (atss * atss) + 3.0 * U * (1.0 + np.abs(ratio).astype(np.float64))
    M, bM = np.vstack([beta, r2[None, :]]), np.vstack([bbeta, br2[None, :]])
    ref = dict(coef=beta, r2=r2, weight=W, deficient=0, moments=moments, ambiguous=0)
    bound = dict(coef=bbeta, r2=br2)
    r, bd = sc.summarise(M, bM)
    ref["mean"], ref["m2"], bound["mean"], bound["m2"] = r["mean"], r["m2"], bd["mean"], bd["m2"]
    if Q:
        ref["quantiles"] = qc.type7(M, probs).astype(np.float64)
        bound["quantiles"] = qc.bound(M.astype(np.float64), bM, Q)
    if threshold is not None:
        th = LD(threshold)
        ref["p_above"] = (M > th).sum(axis=1) / float(S)
        near = np.abs(M - th).astype(np.float64) <= BOUND_FACTOR * bM
        ref["ambiguous"] = 0 if np.isinf(threshold) else int(near.sum())
    return ref, bound


def design_matrix(rows, K, seed=0, intercept=True):
    """A well-conditioned test design: an intercept (where asked for) beside standard normal columns."""
    g = np.random.default_rng(1000 + seed)
    A = g.standard_normal((rows, K))
    if intercept:
        A[:, 0] = 1.0
    return A


def check_inputs(ref, bound, what=""):
    """What makes a comparison within the bounds mean something: cond(G) <= 1e4 and the largest bound of r2 <= 1e-6."""
    cond = float(np.linalg.cond(ref["moments"]["G"].astype(np.float64)))
    worst = float(np.nanmax(bound["r2"]))
    assert cond <= 1e4, f"{what}: cond(G) = {cond:.3g}"
    assert worst <= 1e-6, f"{what}: the largest bound of r2 is {worst:.3g}"
    return cond, worst


def assert_projection(got, ref, bound, what, report=print):
    """A Sampler.predict_projection result (scale_columns=False) against model(): the same flag; answered: every floating output within BOUND_FACTOR x
    its bound, W and p_above exactly; otherwise NaN everywhere.  The ratios are printed before they are asserted."""
    info = got["info"]
    assert got["deficient"] == ref["deficient"] == info["deficient"], (what, got["deficient"], ref["deficient"], info)
    assert got["weight"] == ref["weight"], f"{what}: W is not the host's sum in row order"
    ratios = {}
    if ref["deficient"]:
        for key in FLOATS + ("p_above",):
            if got.get(key) is not None:
                assert np.all(np.isnan(got[key])), f"{what}: {key} is not NaN everywhere although the call has no answer"
        report(f"predict_projection {what}: no answer ({ref['deficient']}), NaN everywhere")
        return ratios
    for key in FLOATS:
        if key in ref and got.get(key) is not None:
            g, r = np.asarray(got[key]), np.asarray(ref[key])
            assert g.shape == r.shape, (what, key, g.shape, r.shape)
            assert np.array_equal(np.isnan(g), np.isnan(r.astype(np.float64))), f"{what}: {key} has NaN in other places than the model"
            ok = ~np.isnan(g)
            ratios[key] = bound_ratio(g[ok], r[ok], bound[key][ok])
    report(f"predict_projection {what}: route {info['route']}, {info['chunks']} chunk(s) of {info['rows_per_chunk']} rows, K = {info['columns']}, "
           f"{info['draws']} draws; max |device - model| / bound: " + ", ".join(f"{k} {r:.3g}" for k, r in ratios.items()))
    for key, r in ratios.items():
        assert r <= BOUND_FACTOR, f"{what}: {key} is {r:.3g} x the derived bound (allowed: {BOUND_FACTOR:g})"
    if "p_above" in ref:
        assert ref["ambiguous"] == 0, f"{what}: {ref['ambiguous']} (row, draw) pair(s) lie within their bound of the threshold: choose another threshold"
        assert np.array_equal(got["p_above"], ref["p_above"], equal_nan=True), f"{what}: p_above differs from the model's exact count"
    return ratios


def padded_columns(K):
    return 8 if K <= 8 else 16 if K <= 16 else 32


def device_bytes_formula(value_bytes, rows, S, K, C, weights=False, mean=True, m2=True, p_above=False, Q=0):
    """the device memory of one call (every allocation at least 16 bytes).  `value_bytes`: what the value kernel's inputs and the
    chunk's scratch take (quantile_cases / contrast_cases.device_bytes_formula without outputs).  No term grows with rows x S beyond the chunk."""
    L = K + 1
    sizes = [8 * rows * padded_columns(K), 8 * -(-C // SLAB) * (K + 2) * max(S, K), 8 * (K + 2) * K, 8 * (K + 2) * S, 8 * L * S, 8 * (L + 1), 8, 8 * L]
    sizes += [8 * rows] * bool(weights) + [8 * L] * (int(bool(mean)) + int(bool(m2)) + int(bool(p_above)))
    if Q:
        sizes += [8 * Q, 8 * Q * L]
    return value_bytes + sum(max(16, t) for t in sizes)
