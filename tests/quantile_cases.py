"""s4b_predict_quantiles (stan4bart_amd/csrc/dev_quantile.inc over dev_readout.inc: k_predict_values<staged / global>, k_row_quantiles) — the model and the bound shared
by tests/test_predict_quantiles.py (CPU) and tests/test_gpu_predict_quantiles.py (GPU).

The reference is numpy on the FULL [rows x pooled draws] matrix, at shapes where the matrix is small: summary_cases.model(...)["v"] per sampler (the
value of predict_summary: predict_bart's fits plus the linear parts in long double, Phi through math.erfc), the samplers concatenated in pooling
order, every row sorted, and R's type 7 in np.longdouble in the shape the device forms it:
    h = p (S - 1),  lo = floor(h),  hi = min(lo + 1, S - 1),  g = h - lo,  q = x(lo) + g (x(hi) - x(lo)).

Bound of an entry (u = 2^-53; the tests allow readout_cases.BOUND_FACTOR x the bound, for the reference's own roundings; no measured constant):
    max_k bound_v[i, k] + u (S (vmax_i - vmin_i) + 4 max_k |v[i, k]|)
  - an order statistic, and a convex combination of two, moves by at most the largest perturbation of the values: max_k bound_v[i, k], the bound
    of summary_cases.model for the device's v;
  - q is continuous and piecewise linear in h with slope at most the row's range vmax - vmin, and the device's h = p (S - 1) carries one rounding of
    a number no larger than S: u S (vmax - vmin).  Continuity makes "lo off by one next to an integer h" harmless: nothing is excluded;
  - the interpolation is a difference, a product and a sum of numbers no larger than 2 max |v|: three roundings, counted as 4 u max |v|."""
import numpy as np

import summary_cases as sc
from readout_cases import BOUND_FACTOR, U, bound_ratio  # noqa: F401

LD = np.longdouble


def type7(v, probs):
    """The quantiles of every row of `v` [rows x S] by the device's formula in long double: [Q x rows] long double."""
    v = np.asarray(v, dtype=LD)
    rows, S = v.shape
    xs = np.sort(v, axis=1)
    out = np.zeros((len(probs), rows), dtype=LD)
    for j, p in enumerate(np.asarray(probs, dtype=np.float64)):
        h = LD(p) * LD(S - 1)
        lo = min(int(np.floor(h)), S - 1)
        hi = min(lo + 1, S - 1)
        out[j] = xs[:, lo] + (h - LD(lo)) * (xs[:, hi] - xs[:, lo])
    return out


def bound(v, bv, n_probs):
    """The derived bound of the module docstring for every entry: [Q x rows] float64."""
    v = np.asarray(v, dtype=np.float64)
    S = v.shape[1]
    b = np.asarray(bv).max(axis=1) + U * (S * (v.max(axis=1) - v.min(axis=1)) + 4.0 * np.abs(v).max(axis=1))
    return np.repeat(b[None, :], n_probs, axis=0)


def model(parts, probs, link=0, offset=None, dense=None, ell_index=None, ell_value=None):
    """`parts`: per pooled sampler, in pooling order, dict(bart [rows x draws], dense_coef, ell_coef) — the coefficient tables of that sampler.
    Returns (quantiles [Q x rows] float64, bound [Q x rows], v [rows x S] float64, bound_v)."""
    vs, bs = [], []
    for p in parts:
        ref, bd = sc.model(p["bart"], offset, dense, p.get("dense_coef"), ell_index, ell_value, p.get("ell_coef"), link=link)
        vs.append(ref["v"])
        bs.append(np.broadcast_to(bd["v"], ref["v"].shape))
    v, bv = np.concatenate(vs, axis=1), np.concatenate(bs, axis=1)
    return type7(v, probs).astype(np.float64), bound(v, bv, len(probs)), v, bv


def assert_quantiles(got, ref, bd, what, report=print):
    """A Sampler.predict_quantiles result against model(): every entry within BOUND_FACTOR x its bound, none left out.  The ratio is printed before
    it is asserted."""
    assert got["quantiles"].shape == ref.shape, (what, got["quantiles"].shape, ref.shape)
    r = bound_ratio(got["quantiles"], ref, bd)
    info = got["info"]
    report(f"predict_quantiles {what}: route {info['route']}, {info['chunks']} chunk(s) of {info['rows_per_chunk']} rows, {info['rows_per_sort']} row(s) per sort "
           f"workgroup at {info['padded_draws']} padded draws, max |device - model| / bound = {r:.3g}")
    assert r <= BOUND_FACTOR, f"{what}: {r:.3g} x the derived bound (allowed: {BOUND_FACTOR:g})"
    return r


def device_bytes_formula(P, rows, nodes, S, T, offset, M, E, q, C, Q):
    """the device memory of one call (every allocation at least 16 bytes).  The only rows-times-draws term is the chunk's: 8 C S."""
    sizes = [2 * P * rows, 24 * nodes, 8 * S * T, 16 * S, 8 * C * S, 8 * Q * rows, 8 * Q]          # binned rows, nodes, tree starts, scales, values, quantiles, probs
    if offset:
        sizes.append(8 * rows)
    if M:
        sizes += [8 * rows * M, 8 * S * M]
    if E:
        sizes += [4 * rows * E, 8 * rows * E, 8 * S * q]
    return sum(max(16, t) for t in sizes)
