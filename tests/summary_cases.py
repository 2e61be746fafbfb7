"""s4b_predict_summary (stan4bart_amd/csrc/dev_summary.inc over dev_readout.inc: k_predict_summary<staged / global>, k_summary_fold) — the model, the bounds and the
inputs shared by tests/test_predict_summary.py (CPU) and tests/test_gpu_predict_summary.py (GPU).

The reference is numpy on the FULL [rows x draws] matrix, at shapes where the matrix is small: predict_bart of the same sampler supplies the BART fits
(it is held to the numpy walk by tests/test_gpu_readout.py), the linear parts are added in the stated order in np.longdouble, Phi is
0.5 * math.erfc(-z / sqrt 2), and mean, sum (v - mean)^2 and the weighted row sums are taken in long double.

Bounds (u = 2^-53; the tests allow readout_cases.BOUND_FACTOR x the bound of an entry, for the reference's own roundings):
  z     The BART fit is predict_bart's value bit for bit (asserted separately), so it enters as an exact term.  The device then adds the offset (one
        rounding) and, per dense column and per ELL entry, a product and a sum (two roundings, one if contracted).  Every partial sum is at most
        A = |bart| + |offset| + sum |dense * coef| + sum |value * coef| up to first order, so |error(z)| <= ops * u * A with
        ops = [offset] + 2 M + 2 E' (E' the row's entries that are not padding).  ops = 0: z is exact.
  Phi   v = 0.5 * erfc(-z * (1 / sqrt 2)): the rounded constant and the product add 2 u |z| <= 2 u A to the error of the argument (counted as two
        more operations of z), the derivative of Phi is phi(z), and erfc itself returns c ulps: |error(v)| <= phi(z) * bound(z) + c * u.  No
        document under the ROCm installation states an accuracy for erfc, so c was measured on the first run on an MI355X against math.erfc at
        the tests' own arguments (the binary and Gaussian cases of the GPU tests, link 1, no linear parts: z is then exactly predict_bart's value):
        the largest |device - reference| / u was ERFC_C_MEASURED = 1.5 (three quarters of an ulp of a value in [0.5, 1)); ERFC_C is twice that
        (DESIGN.md 5.5).
  mean  Welford's update mean += (v - mean) / k: the errors of v average, and every step rounds a difference, a quotient and a sum of numbers no
        larger than 2 max |v|; a step's error is carried into later means with factor (1 - 1 / k) <= 1, so
        |error(mean)| <= mean_k bound(v_k) + 4 S u max_k |v_k|.
  m2    sum_k (v_k - mean)^2 moves by 2 |v_k - mean| e_k + e_k^2 when v_k - mean moves by e_k <= bound(v_k) + bound(mean); the update
        m2 += d * (v - mean) adds non-negative terms whose sum is m2, each formed with three roundings and added with one:
        |error(m2)| <= sum_k (2 |v_k - mean| e_k + e_k^2) + (S + 4) u m2.
  average[k, g] = sum_i w[g, i] v[i, k]: the errors of v weighted, plus one rounding per product and per addition (wave butterfly, waves, tiles,
        workgroups: fewer than `rows` additions on any path): |error| <= sum_i |w| bound(v) + rows * u * sum_i |w v|."""
import math

import numpy as np

from readout_cases import BOUND_FACTOR, U, bound_ratio  # noqa: F401  (BOUND_FACTOR: the allowance of every comparison here)

ERFC_C_MEASURED = 1.5          # largest |device Phi - math.erfc Phi| / u over the tests' arguments on an MI355X (first run); see the docstring
ERFC_C = 2.0 * ERFC_C_MEASURED
LD = np.longdouble


def phi_cdf(z):
    """0.5 * erfc(-z / sqrt 2) through math.erfc, elementwise, for an array of any float type."""
    z = np.asarray(z)
    return np.array([0.5 * math.erfc(-float(t) / math.sqrt(2.0)) for t in z.ravel()], dtype=np.float64).reshape(z.shape)


def phi_pdf(z):
    z = np.asarray(z, dtype=np.float64)
    return np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def welford(v):
    """(mean, m2) along the last axis by Welford's update in order — the device's recurrence, in the precision of `v`."""
    v = np.asarray(v)
    mean = np.zeros(v.shape[:-1], dtype=v.dtype)
    m2 = np.zeros(v.shape[:-1], dtype=v.dtype)
    for k in range(v.shape[-1]):
        d = v[..., k] - mean
        mean = mean + d / v.dtype.type(k + 1)
        m2 = m2 + d * (v[..., k] - mean)
    return mean, m2


def chan_pool(parts):
    """(count, mean, m2) of several samples pooled pairwise (Chan, Golub, LeVeque) — what Stan4bartFit._pool_chains must compute."""
    n, mean, m2 = parts[0]
    for nb, mb, m2b in parts[1:]:
        d = mb - mean
        tot = n + nb
        mean, m2, n = mean + d * nb / tot, m2 + m2b + d * d * n * nb / tot, tot
    return n, mean, m2


def model(bart, offset=None, dense=None, dense_coef=None, ell_index=None, ell_value=None, ell_coef=None, link=0, weights=None, erfc_c=None):
    """The reference and its bounds.  `bart` [rows x S] (predict_bart); the other arguments as Sampler.predict_summary takes them.
    Returns dict(v, mean, m2, average [S x G]) as float64 and dict(v, mean, m2, average) of bounds, float64."""
    bart = np.asarray(bart, dtype=np.float64)
    rows, S = bart.shape
    z = bart.astype(LD)
    A = np.abs(z)
    ops = np.zeros((rows, 1))
    if offset is not None:
        o = np.asarray(offset, dtype=np.float64).astype(LD)[:, None]
        z = z + o
        A = A + np.abs(o)
        ops = ops + 1
    if dense is not None and np.asarray(dense).shape[1]:
        d, c = np.asarray(dense, dtype=np.float64).astype(LD), np.asarray(dense_coef, dtype=np.float64).astype(LD)
        for j in range(d.shape[1]):
            t = d[:, j][:, None] * c[:, j][None, :]
            z = z + t
            A = A + np.abs(t)
        ops = ops + 2 * d.shape[1]
    if ell_index is not None and np.asarray(ell_index).shape[1]:
        ix, ev, ec = np.asarray(ell_index), np.asarray(ell_value, dtype=np.float64).astype(LD), np.asarray(ell_coef, dtype=np.float64).astype(LD)
        for e in range(ix.shape[1]):
            on = ix[:, e] >= 0
            t = np.zeros((rows, S), dtype=LD)
            t[on] = ev[on, e][:, None] * ec[:, ix[on, e]].T
            z = z + t
            A = A + np.abs(t)
            ops = ops + 2 * on[:, None]
    bz = (ops * U * A).astype(np.float64)
    if link:
        c = ERFC_C if erfc_c is None else erfc_c
        v = phi_cdf(z).astype(LD)
        bv = phi_pdf(z.astype(np.float64)) * ((ops + 2) * U * A).astype(np.float64) + c * U
    else:
        v, bv = z, bz
    return summarise(v, bv, weights)


def summarise(v, bv, weights=None):
    """mean, m2 over the draws and weighted row sums of the matrix `v` [rows x S] (long double) whose entries the device knows to within `bv`:
    (reference values, bounds), by the rules of the module docstring."""
    v = np.asarray(v, dtype=LD)
    rows, S = v.shape
    mean = v.sum(axis=1) / LD(S)
    dev = v - mean[:, None]
    m2 = (dev * dev).sum(axis=1)
    vmax = np.abs(v).max(axis=1).astype(np.float64)
    bmean = bv.mean(axis=1) + 4.0 * S * U * vmax
    e = bv + bmean[:, None]
    bm2 = (2.0 * np.abs(dev).astype(np.float64) * e + e * e).sum(axis=1) + (S + 4.0) * U * m2.astype(np.float64)
    ref = dict(v=v.astype(np.float64), mean=mean.astype(np.float64), m2=m2.astype(np.float64))
    bound = dict(v=bv, mean=bmean, m2=bm2)
    if weights is not None:
        w = np.asarray(weights, dtype=np.float64).astype(LD)          # [G x rows]
        ref["average"] = (w @ v).T.astype(np.float64)                 # [S x G]
        bound["average"] = ((np.abs(w).astype(np.float64) @ bv) + rows * U * (np.abs(w) @ np.abs(v)).astype(np.float64)).T
    return ref, bound


def assert_summary(got, ref, bound, what, report=print):
    """mean, m2 and average of a Sampler.predict_summary result against model(): every entry within BOUND_FACTOR x its bound.  The ratios are
    printed before they are asserted."""
    ratios = {}
    for key in ("mean", "m2", "average"):
        if key in ref:
            assert got[key].shape == ref[key].shape, (what, key, got[key].shape, ref[key].shape)
            ratios[key] = bound_ratio(got[key], ref[key], bound[key])
    report(f"predict_summary {what}: route {got['info']['route']}, {got['info']['workgroups']} workgroup(s), max |device - model| / bound: "
           + ", ".join(f"{k} {r:.3g}" for k, r in ratios.items()))
    for key, r in ratios.items():
        assert r <= BOUND_FACTOR, f"{what}: {key} is {r:.3g} x the derived bound (allowed: {BOUND_FACTOR:g})"
    return ratios


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------------
def linear_parts(rows, S, M, E, q=7, seed=0, scale=1.0):
    """Dense and ELL parts for `rows` rows and S draws: M dense columns, E ELL entries per row over q coefficient columns with ragged padding (row i
    keeps its first i mod (E + 1) entries, from none to all E; the first and the last row keep all), the indices 0 and q - 1 both in use."""
    g = np.random.default_rng(5000 + seed)
    out = {}
    if M:
        out["dense"] = g.normal(size=(rows, M)) * scale
        out["dense_coef"] = g.normal(size=(S, M))
    if E:
        ix = g.integers(0, q, size=(rows, E)).astype(np.int32)
        ix[0, 0], ix[rows - 1, E - 1] = 0, q - 1
        keep = np.arange(rows) % (E + 1)                              # entries kept in front: E = 1 alternates padding / entry
        for e in range(E):
            drop = e >= keep
            drop[0] = drop[rows - 1] = False
            ix[drop, e] = -1
        out["ell_index"], out["ell_value"], out["ell_coef"] = ix, g.normal(size=(rows, E)) * scale, g.normal(size=(S, q))
    return out


def weight_vectors(rows, G, seed=0):
    """G weight vectors: the sample average 1 / rows, a subgroup indicator over its count, one with zeros and negative entries, then random ones."""
    g = np.random.default_rng(6000 + seed)
    w = g.normal(size=(G, rows))
    w[0] = 1.0 / rows
    if G > 1:
        sub = (np.arange(rows) % 3 == 0).astype(np.float64)
        w[1] = sub / max(1.0, sub.sum())
    if G > 2:
        w[2] = np.where(np.arange(rows) % 2 == 0, 0.0, -np.abs(w[2]))
    return w


def random_terms(seed, n_rows=40):
    """Grouping terms of a fitted model and of new rows for the ELL builder: an intercept-and-two-slopes term, an intercept term, a slope term; the new
    rows carry seen and unseen levels.  Returns (fit terms, new terms, q)."""
    from stan4bart_amd import GroupTerm
    g = np.random.default_rng(7000 + seed)
    ls, ps = (4, 6, 3), (3, 1, 2)
    fit_terms = []
    for t, (l, p) in enumerate(zip(ls, ps)):
        lev = np.r_[np.arange(1, l + 1), g.integers(1, l + 1, 10)]
        fit_terms.append(GroupTerm(lev, g.normal(size=(len(lev), p - 1)) if p > 1 else None, f"g.{t + 1}"))
    new_terms = []
    for t, (l, p) in enumerate(zip(ls, ps)):
        lev = g.integers(1, l + 3, n_rows)                            # levels l + 1, l + 2 are unseen
        lev[0], lev[1] = 1, l + 2
        new_terms.append(GroupTerm(lev, g.normal(size=(n_rows, p - 1)) if p > 1 else None, f"g.{t + 1}"))
    return fit_terms, new_terms, sum(l * p for l, p in zip(ls, ps))


def fake_fit(seed, n_iter=5, n_chain=2, family="gaussian", samplers=()):
    """A Stan4bartFit with random draws and no sampler behind it (random_terms' model, two fixed effects): what the host-side pieces of
    predict_summary need."""
    from stan4bart_amd.generics import Stan4bartFit
    g = np.random.default_rng(8000 + seed)
    fit_terms, new_terms, q = random_terms(seed)
    n_theta = sum(t.p * (t.p + 1) // 2 for t in fit_terms)
    names = ["beta.1", "beta.2"] + [f"b.{j + 1}" for j in range(q)] + [f"theta_L.{j + 1}" for j in range(n_theta)] + ["aux.1"]
    stan = g.normal(size=(len(names), n_iter, n_chain))
    n = len(fit_terms[0].levels)
    fit = Stan4bartFit(family=family, par_names=names, stan=stan, bart_train=np.zeros((n, n_iter, n_chain)), bart_test=None,
                       bart_varcount=np.zeros((3, n_iter, n_chain), dtype=np.int32), warmup=None, X=g.normal(size=(n, 2)), X_means=g.normal(size=2),
                       X_test=None, terms=fit_terms, terms_test=None, offset=None, offset_test=None, offset_type="default",
                       range_bart=np.zeros((2, n_chain)), samplers=list(samplers))
    return fit, new_terms, q
