"""s4b_predict_contrast (stan4bart_amd/csrc/dev_contrast.inc over dev_readout.inc, dev_quantile.inc: k_contrast_values<staged / global>, k_contrast_reduce,
k_contrast_fold, k_row_quantiles) — the model, the bounds and the inputs shared by tests/test_predict_contrast.py (CPU) and
tests/test_gpu_predict_contrast.py (GPU).

The reference is numpy in long double on the FULL [rows x pooled draws] matrices of both arms, at shapes where they are small.  predict_bart of every
pooled sampler at each arm's rows supplies the BART fits; the linear parts are added in long double in summary_cases' order, Phi is summary_cases'
phi_cdf:
    z_a = bart_a + offset_a + sum_j dense_a[:, j] coef[k, j] + sum_e value_a[:, e] ellcoef[k, index_a[:, e]],      d = v(z_1) - v(z_0).

Bound of d(i, k) (u = 2^-53; every comparison allows readout_cases.BOUND_FACTOR x the bound, for the reference's own roundings; no measured constant
but summary_cases.ERFC_C).  T trees per draw, A(k) of them with a rule on a differing column, [lo, hi] the response scale, w = hi - lo (binary
response: w = 1, lo = 0 and no "+ 0.5": there is no rescale), F_a = sum_t |mu_t| at arm a's row over all trees, G_a the same over the affected trees:
  order_a   = (T + 2) u (F_a + 0.5) w + u |lo|: readout_cases' derived term of a T-term leaf sum and its rescale.  predict_bart's value of each arm
              carries it; so does a device sum of the same T terms in another order (link 1).
  link 0    The device forms w (s1 - s0) + (lin1 - lin0).  s_a adds A leaf values from 0.0: at most A roundings of partial sums no larger than G_a;
              the difference and the product add one rounding each of numbers no larger than G_1 + G_0: (A + 2) u w (G_1 + G_0).  lin_a adds only
              the parts that DIFFER between the arms, from the arm's offset: ops_a u L_a with ops = 2 per dense column and per ELL entry that is no
              padding and L_a = |offset_a| + sum |terms| (summary_cases' rule); their difference and the final sum round numbers no larger than
              w (G_1 + G_0) + L_1 + L_0 three times.  The reference's bart_1 - bart_0 adds order_1 + order_0 — except in a draw without an affected
              tree, where both predict_bart values are the same sum of the same leaves and the difference is exactly 0, as the device's is.
                  bound = order_1 + order_0 + (A + 2) u w (G_1 + G_0) + u (ops_1 L_1 + ops_0 L_0) + 3 u (w (G_1 + G_0) + L_1 + L_0)
              Identical arms: every term of the bound is 0, and so must both sides be.
  link 1    z_a = (response(f_a) + shared) + lin_a with f_a the T leaf values in the contrast's order: 2 order_a (the device's and predict_bart's),
              plus (ops + 2) u Z_a for ALL linear parts (ops as above, + 1 for an offset; two more roundings for the two outer sums), Z_a = |bart_a| +
              |offset_a| + sum |terms|.  Through Phi as in summary_cases: phi(z_a) (bound(z_a) + 2 u Z_a) + ERFC_C u per arm, and one rounding of the
              difference: u |d|.
Bounds of the outputs follow summary_cases.summarise(d, bound_d, weights):
  mean      The device adds the S values of a row lane by lane (at most ceil(S / 64) additions), six butterfly steps, one division: fewer roundings
              than Welford's 4 S for every S >= 2, and none at S = 1 — summarise's bound of the mean holds unchanged.
  m2        Two passes: every term (d - mean)^2 with three roundings, ceil(S / 64) + 6 additions: inside summarise's (S + 4) u m2 for S >= 2; exactly 0 at S = 1.
  average   sum_i w[g, i] d[i, k]: the rows of a slab of 64 in row order, the slabs in order: at most min(rows, 64) + ceil(rows / 64) additions and
              one rounding per product on any path, in place of summarise's `rows`:
                  sum_i |w| bound(d) + (min(rows, 64) + ceil(rows / 64) + 1) u sum_i |w d|.
  quantiles quantile_cases.type7 and quantile_cases.bound over d and bound(d)."""
import numpy as np

import quantile_cases as qc
import readout_cases as rc
import summary_cases as sc
from readout_cases import BOUND_FACTOR, U, bound_ratio  # noqa: F401

LD = np.longdouble
SLAB = 64          # rows per workgroup of k_contrast_reduce (CT_SLAB)


def linear(rows, S, offset=None, dense=None, dense_coef=None, ell_index=None, ell_value=None, ell_coef=None):
    """The linear parts of one arm in long double, in summary_cases.model's order: (sum [rows x S], sum of magnitudes [rows x S], ops [rows x 1] — 2 per
    dense column and per ELL entry that is no padding; the offset is not counted here)."""
    z, A, ops = np.zeros((rows, S), dtype=LD), np.zeros((rows, S), dtype=LD), np.zeros((rows, 1))
    if offset is not None:
        o = np.asarray(offset, dtype=np.float64).astype(LD)[:, None]
        z, A = z + o, A + np.abs(o)
    if dense is not None and np.asarray(dense).shape[1]:
        d, c = np.asarray(dense, dtype=np.float64).astype(LD), np.asarray(dense_coef, dtype=np.float64).astype(LD)
        for j in range(d.shape[1]):
            t = d[:, j][:, None] * c[:, j][None, :]
            z, A = z + t, A + np.abs(t)
        ops = ops + 2 * d.shape[1]
    if ell_index is not None and np.asarray(ell_index).shape[1]:
        ix, ev, ec = np.asarray(ell_index), np.asarray(ell_value, dtype=np.float64).astype(LD), np.asarray(ell_coef, dtype=np.float64).astype(LD)
        for e in range(ix.shape[1]):
            on = ix[:, e] >= 0
            t = np.zeros((rows, S), dtype=LD)
            t[on] = ev[on, e][:, None] * ec[:, ix[on, e]].T
            z, A = z + t, A + np.abs(t)
            ops = ops + 2 * on[:, None]
    return z, A, ops


def leaf_sums(trees, x, hit):
    """(F, G) [rows x S]: sum_t |mu_t| at the raw rows `x` over all trees of a draw and over the trees marked in `hit` [S x T] (pd_cases.affected)."""
    S, T = hit.shape
    F, G = np.zeros((len(x), S)), np.zeros((len(x), S))
    for a, _, pos in rc.walk_leaves(trees, x):
        mu = np.abs(trees["value"][pos])
        F[:, a // T] += mu
        if hit[a // T, a % T]:
            G[:, a // T] += mu
    return F, G


def bins(x, cuts):
    """bin_matrix restated: per column the number of cut points strictly below the value.  `cuts`: one ascending vector per column."""
    x = np.asarray(x, dtype=np.float64)
    return np.column_stack([np.searchsorted(np.asarray(c, dtype=np.float64), x[:, j], side="left") for j, c in enumerate(cuts)])


def differing_columns(x1, x0, cuts):
    """The host's rule restated: the columns whose BINS differ in at least one row (two raw values on the same side of every cut do not differ)."""
    return [int(j) for j in np.flatnonzero((bins(x1, cuts) != bins(x0, cuts)).any(axis=0))]


def resolve_arm0(arm1, arm0):
    """Arm 0's row side with every part that was not given taken from arm 1, and which parts differ."""
    full = {k: (arm0.get(k) if arm0.get(k) is not None else arm1.get(k)) for k in ("offset", "dense", "ell_index", "ell_value")}
    differs = dict(offset=arm0.get("offset") is not None, dense=arm0.get("dense") is not None,
                   ell=arm0.get("ell_index") is not None or arm0.get("ell_value") is not None)
    return full, differs


def model(parts, arm1, arm0, T, ranges, binary, link=0, weights=None, probs=()):
    """`parts`: per pooled sampler, in pooling order, dict(bart1, bart0 [rows x draws] (predict_bart at each arm's rows), F1, F0, G1, G0 (leaf_sums),
    n_affected [draws], dense_coef, ell_coef).  `arm1`, `arm0`: dict(offset, dense, ell_index, ell_value), arm 0's parts None where it shares arm 1's.
    Returns (ref, bound): dicts with d [rows x S], mean, m2, average [S x G] (with weights), quantiles [Q x rows] (with probs)."""
    full0, differs = resolve_arm0(arm1, arm0)
    lo, hi = (0.0, 1.0) if binary else (float(ranges[0]), float(ranges[1]))
    w = hi - lo
    half = 0.0 if binary else 0.5
    ds, bs = [], []
    for p in parts:
        rows, S = p["bart1"].shape
        b1, b0 = p["bart1"].astype(LD), p["bart0"].astype(LD)
        order1 = (T + 2) * U * (p["F1"] + half) * w + U * abs(lo)
        order0 = (T + 2) * U * (p["F0"] + half) * w + U * abs(lo)
        tab = dict(dense_coef=p.get("dense_coef"), ell_coef=p.get("ell_coef"))
        L1, Z1, ops1 = linear(rows, S, arm1.get("offset"), arm1.get("dense"), ell_index=arm1.get("ell_index"), ell_value=arm1.get("ell_value"), **tab)
        L0, Z0, ops0 = linear(rows, S, full0["offset"], full0["dense"], ell_index=full0["ell_index"], ell_value=full0["ell_value"], **tab)
        if not link:
            d = (b1 - b0) + (L1 - L0)
            # the device's linear terms: the differing parts alone
            pick = lambda arm: dict(offset=arm["offset"] if differs["offset"] else None, dense=arm["dense"] if differs["dense"] else None,
                                    ell_index=arm["ell_index"] if differs["ell"] else None, ell_value=arm["ell_value"] if differs["ell"] else None)
            _, D1, o1 = linear(rows, S, **pick(arm1), **tab)
            _, D0, o0 = linear(rows, S, **pick(full0), **tab)
            G = w * (p["G1"] + p["G0"])
            nA = np.asarray(p["n_affected"])[None, :]
            # (a draw without an affected tree: both predict_bart values are the same sum of the same leaves — the BART terms vanish on both sides)
            bd = ((nA > 0) * (order1 + order0) + (nA + 2) * U * G + U * (o1 * D1 + o0 * D0).astype(np.float64) + 3.0 * U * (G + (D1 + D0).astype(np.float64)))
        else:
            z1, z0 = b1 + L1, b0 + L0
            off = 1 if arm1.get("offset") is not None else 0
            A1, A0 = (np.abs(b1) + Z1).astype(np.float64), (np.abs(b0) + Z0).astype(np.float64)
            bz1 = 2.0 * order1 + (ops1 + off + 2) * U * A1
            bz0 = 2.0 * order0 + (ops0 + off + 2) * U * A0
            v1, v0 = sc.phi_cdf(z1).astype(LD), sc.phi_cdf(z0).astype(LD)
            d = v1 - v0
            bd = (sc.phi_pdf(z1.astype(np.float64)) * (bz1 + 2.0 * U * A1) + sc.phi_pdf(z0.astype(np.float64)) * (bz0 + 2.0 * U * A0) + 2.0 * sc.ERFC_C * U
                  + U * np.abs(d).astype(np.float64))
        ds.append(d)
        bs.append(np.broadcast_to(bd, d.shape))
    d, bd = np.concatenate(ds, axis=1), np.concatenate(bs, axis=1).astype(np.float64)
    ref, bound = sc.summarise(d, bd, weights)
    ref["d"], bound["d"] = ref.pop("v"), bound.pop("v")
    if weights is not None:
        rows = d.shape[0]
        wt = np.asarray(weights, dtype=np.float64)
        adds = min(rows, SLAB) + -(-rows // SLAB) + 1
        bound["average"] = ((np.abs(wt) @ bd) + adds * U * (np.abs(wt).astype(LD) @ np.abs(d)).astype(np.float64)).T
    if len(probs):
        ref["quantiles"] = qc.type7(d, probs).astype(np.float64)
        bound["quantiles"] = qc.bound(d.astype(np.float64), bd, len(probs))
    return ref, bound


def assert_contrast(got, ref, bound, what, report=print, keys=("mean", "m2", "average", "quantiles")):
    """A Sampler.predict_contrast result against model(): every entry of every output within BOUND_FACTOR x its bound.  The ratios are printed before
    they are asserted."""
    ratios = {}
    for key in keys:
        if key in ref and got.get(key) is not None and np.size(got[key]):
            assert got[key].shape == ref[key].shape, (what, key, got[key].shape, ref[key].shape)
            ratios[key] = bound_ratio(got[key], ref[key], bound[key])
    info = got["info"]
    report(f"predict_contrast {what}: route {info['route']}, {info['chunks']} chunk(s) of {info['rows_per_chunk']} rows, D {info['differing_columns']}, affected trees at most "
           f"{info['largest_affected']} / in all {info['total_affected']}; max |device - model| / bound: " + ", ".join(f"{k} {r:.3g}" for k, r in ratios.items()))
    for key, r in ratios.items():
        assert r <= BOUND_FACTOR, f"{what}: {key} is {r:.3g} x the derived bound (allowed: {BOUND_FACTOR:g})"
    return ratios


def brute_force(predict_bart1, predict_bart0, probs, weights):
    """Plain numpy, double precision, link 0, no linear part: the host way a user would write."""
    d = predict_bart1 - predict_bart0
    return dict(mean=d.mean(axis=1), m2=((d - d.mean(axis=1, keepdims=True)) ** 2).sum(axis=1), average=(np.asarray(weights) @ d).T,
                quantiles=np.quantile(d, probs, axis=1) if len(probs) else np.zeros((0, len(d))))


def device_bytes_formula(P, rows, nodes, S, T, C, D=0, offset=False, M=0, E=0, q=0, offset0=False, dense0=False, ell_index0=False, ell_value0=False,
                         per_row=True, G=0, Q=0):
    """the device memory of one call (every allocation at least 16 bytes).  offset, M, E: the arm-1 parts that are EVALUATED (under link 0
    only those whose arm-0 side was given).  The only rows-times-draws term is the chunk's: 8 C S."""
    sizes = [2 * P * rows, 24 * nodes, 8 * S * T, 16 * S, 4 * S * T, 4 * S, 8 * C * S]          # binned rows, nodes, tree starts, scales, tree order, unaffected counts, values
    if offset:
        sizes.append(8 * rows)
    if M:
        sizes += [8 * rows * M, 8 * S * M]
    if E:
        sizes += [4 * rows * E, 8 * rows * E, 8 * S * q]
    if D:
        sizes.append(2 * D * rows)
    sizes += [8 * rows] * bool(offset0) + [8 * rows * M] * bool(dense0) + [4 * rows * E] * bool(ell_index0) + [8 * rows * E] * bool(ell_value0)
    if per_row:
        sizes += [8 * rows, 8 * rows]
    if G:
        sizes += [8 * G * rows, 8 * -(-C // SLAB) * S * G, 8 * S * G]
    if Q:
        sizes += [8 * Q, 8 * Q * rows]
    return sum(max(16, t) for t in sizes)
