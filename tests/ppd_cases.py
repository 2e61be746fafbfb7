"""s4b_predict_ppd (stan4bart_amd/csrc/dev_ppd.inc: k_predict_values<staged / global> unchanged, k_ppd_rows; the deviate: philox_normal, csrc/philox.hpp;
DESIGN.md 5.9) — the model and the bounds shared by tests/test_predict_ppd.py (CPU) and tests/test_gpu_predict_ppd.py (GPU).

The reference is numpy on the FULL [rows x pooled draws] matrix, at shapes where the matrix is small:
  z      summary_cases.model(..., link=0)["v"] per pooled sampler, concatenated in pooling order, with its bound bound_z;
  sd     fl(sigma[k] * row_scale[i]) in DOUBLE: the one product the device forms too (correctly rounded on both sides, so sd is an exact input);
  e      latent_par_cases.philox4x32_10 / u53 at counter {row low, row high, draw, PPD_TAG}, key {low, high}; sqrt(-2 log u1) cos(2 pi u2) in long
         double with 2 pi the double 6.283185307179586 (philox.hpp's);
  y_rep  z + sd e in long double; quantile_cases.type7;
  l, lpd, lmean, lm2, pit in long double from the definitions of include/stan4bart_amd.h; Phi is summary_cases.phi_cdf (math.erfc of -t / sqrt 2: for a
         negative t the complementary error function of a positive argument, formed directly, so the lower tail keeps its relative accuracy).

BOUNDS, u = 2^-53, derived and not fitted; the tests allow readout_cases.BOUND_FACTOR x the bound of an entry and compare every entry.
k_f is the error of the library function f in ulps (k ulps is at most 2 k u relative): latent_par_cases.DEVICE — log 1, exp 1, sin / cos 2, sqrt 1,
ASSUMED there and assumed here (the figures of the HIP programming guide's table of double-precision math functions; nothing installed states them) —
and GLIBC for the host comparison.  erfc: summary_cases.ERFC_C ulps, the figure that module uses for link 1.
  e       latent_par_cases' normal branch: |error(e)| <= u (2 pi rad + (k_log + 2 k_sqrt + 2 k_trig + 1) |e|), rad = sqrt(-2 log u1).
  y_rep   the product sd e and the sum round once each (or once together):  bound_z + sd bound_e + u (|z| + 2 sd |e|).
  q       an order statistic moves by at most the largest perturbation of its row; then quantile_cases' two interpolation terms (quantile_cases.bound).
  r       (y - z) / sd: a difference and a quotient:  |error(r)| <= (bound_z + u |y - z|) / sd + u |r|.
  l       link 0, (-c - log sd) - r^2 / 2 with c = log(2 pi) / 2: the rounded constant u c, the logarithm 2 k_log u |log sd|, the difference
          u (c + |log sd|), the square |r| e_r + e_r^2 / 2 + u r^2 / 2 (the half is exact), the last difference u |l|.
          link 1, log Phi(t), t = +-z, Phi = 0.5 erfc(-t / sqrt 2): the argument moves by bound_z + 2 u |t| (rounded constant, product), which moves
          Phi by phi(t) times that — relative to Phi: the inverse Mills ratio phi / Phi —, erfc returns ERFC_C ulps: 2 ERFC_C u relative (the case
          builder asserts |z| <= 8: erfc stays far from the subnormal range, where an error in ulps says nothing about the relative error); the
          logarithm turns a relative error rho of its argument into rho / (1 - rho) and adds 2 k_log u |l|.
  tree    the draw sums of a row: a lane adds ceil(S / (64 W)) terms in order, the butterfly six more, the W waves of a row W - 1 more
          (W = 1, 2, 4 waves per row at up to 1024, 2048, more padded draws: dev_ppd.inc), so a sum of terms of one sign carries D u relative,
          D = ceil(S / (64 W)) + 6 + (W - 1)   (`tree_depth`).
  lpd     log-sum-exp is 1-Lipschitz in the sup norm of l: max_k bound_l.  The terms t_k = exp(l_k - m): the difference rounds (u |l_k - m|, weighted
          by t_k / sum t: computed per row), exp 2 k_exp u, the sum D u — all relative to sum t, which the logarithm takes over (sum t >= 1) and
          adds 2 k_log u |log sum t|; m + log sum t rounds u |m + log sum t|; log S: 2 k_log u log S; the last difference u |lpd|.
  lmean   mean_k bound_l + (D + 1) u max_k |l|  (the sum, the quotient).
  lm2     summary_cases' m2 argument with this tree: e_k = bound_l + bound_lmean + u |l_k - lmean|;
          sum_k (2 |l_k - lmean| e_k + e_k^2) + (D + 4) u lm2.
  pit     Phi(r) moves by phi(r) (e_r + 2 u |r|) + ERFC_C u (summary_cases' link-1 bound of Phi); the mean adds (D + 1) u (values <= 1)."""
import math
import os
import re

import numpy as np

import latent_par_cases as lp
import quantile_cases as qc
import summary_cases as sc
from readout_cases import BOUND_FACTOR, U, bound_ratio  # noqa: F401

LD = np.longdouble
C_HALF_LOG_2PI = 0.91893853320467274178
_M32 = np.uint64(0xFFFFFFFF)


def header_constants():
    """PPD_TAG and TN_MAX_ATTEMPTS READ from philox.hpp, with the counter line of philox_normal asserted to still be there."""
    phx = open(os.path.join(lp.CSRC, "philox.hpp")).read()
    assert "const Philox4 c = {{(uint32_t)row, (uint32_t)(row >> 32), draw, PPD_TAG}};" in phx, "the counter layout of philox_normal changed"
    assert "return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);" in phx
    tag = int(re.search(r"constexpr uint32_t PPD_TAG = (0x[0-9A-Fa-f]+)u;", phx).group(1), 16)
    attempts = 1 << int(re.search(r"constexpr int TN_MAX_ATTEMPTS = 1 << (\d+);", phx).group(1))
    return tag, attempts


PPD_TAG = header_constants()[0]


def noise(key, rows, draws, figures=None):
    """e [len(rows) x len(draws)] in long double for the row indices `rows` and the pooled draw indices `draws` under the 64-bit `key`, and its bound
    under `figures` (default: latent_par_cases.DEVICE)."""
    k = lp.DEVICE if figures is None else figures
    i = np.asarray(rows, dtype=np.uint64)[:, None]
    d = np.asarray(draws, dtype=np.uint64)[None, :]
    r = lp.philox4x32_10(i & _M32, i >> np.uint64(32), d, PPD_TAG, int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF)
    u1, u2 = lp.u53(r[0], r[1]), lp.u53(r[2], r[3])
    rad = np.sqrt(LD(-2.0) * np.log(u1.astype(LD)))
    e = rad * np.cos(LD(lp.TWO_PI) * u2.astype(LD))
    be = U * (lp.TWO_PI * rad.astype(np.float64) + (k["log"] + 2 * k["sqrt"] + 2 * k["trig"] + 1) * np.abs(e).astype(np.float64))
    return e, be


def tree_depth(S):
    """D of the module docstring: the additions on the longest path of a row's draw sum in k_ppd_rows."""
    sp = 1 << max(0, int(S) - 1).bit_length()
    R = max(1, 4096 // sp)
    W = 1 if R >= 4 else 4 // R
    return -(-int(S) // (64 * W)) + 6 + (W - 1)


def _phi_ld(t):
    return sc.phi_cdf(t).astype(LD)


def pooled_z(parts, offset=None, dense=None, ell_index=None, ell_value=None):
    """(z [rows x S] float64 — the long-double sums rounded once —, bound_z) of the pooled samplers `parts` (quantile_cases.model's `parts`)."""
    zs, bs = [], []
    for p in parts:
        ref, bd = sc.model(p["bart"], offset, dense, p.get("dense_coef"), ell_index, ell_value, p.get("ell_coef"), link=0)
        zs.append(ref["v"])
        bs.append(np.broadcast_to(bd["v"], ref["v"].shape))
    return np.concatenate(zs, axis=1), np.concatenate(bs, axis=1)


def score(z, bz, y, sd, link, figures=None):
    """The four row reductions and their bounds from z [rows x S] (known to within bz), y [rows], sd [rows x S] (link 0): (ref, bound) dicts with
    lpd, lmean, lm2 and (link 0) pit; ref also carries l."""
    k = lp.DEVICE if figures is None else figures
    z = np.asarray(z, dtype=np.float64)
    rows, S = z.shape
    D = tree_depth(S)
    yv = np.asarray(y, dtype=np.float64)[:, None]
    zl = z.astype(LD)
    if link:
        assert np.all(np.abs(z) <= 8.0), "link 1: |z| <= 8 keeps erfc where its error in ulps is a relative error"
        assert np.all((yv == 0.0) | (yv == 1.0))
        t = np.where(yv > 0.0, z, -z)
        Phi = _phi_ld(t)
        l = np.log(Phi)
        mills = (sc.phi_pdf(t) / Phi.astype(np.float64))
        rho = mills * (bz + 2.0 * U * np.abs(t)) + 2.0 * sc.ERFC_C * U
        bl = rho / (1.0 - rho) + 2.0 * k["log"] * U * np.abs(l).astype(np.float64)
        r = er = None
    else:
        sdl = np.asarray(sd, dtype=np.float64).astype(LD)
        sdf = sdl.astype(np.float64)
        r = (yv.astype(LD) - zl) / sdl
        ra = np.abs(r).astype(np.float64)
        er = (bz + U * np.abs(yv - z)) / sdf + U * ra
        lsd = np.log(sdl)
        l = (LD(-C_HALF_LOG_2PI) - lsd) - LD(0.5) * r * r
        alsd = np.abs(lsd).astype(np.float64)
        bl = (U * C_HALF_LOG_2PI + 2.0 * k["log"] * U * alsd + U * (C_HALF_LOG_2PI + alsd) + ra * er + 0.5 * er * er + 0.5 * U * ra * ra
              + U * np.abs(l).astype(np.float64))
    la = np.abs(l).astype(np.float64)
    m = l.max(axis=1)
    t_k = np.exp(l - m[:, None])
    st = t_k.sum(axis=1)
    lpd = m + np.log(st) - np.log(LD(S))
    rel = U * ((t_k * np.abs(l - m[:, None])).sum(axis=1) / st).astype(np.float64) + (D + 2.0 * k["exp"]) * U
    blpd = (bl.max(axis=1) + rel + 2.0 * k["log"] * U * np.abs(np.log(st)).astype(np.float64) + U * np.abs(m + np.log(st)).astype(np.float64)
            + 2.0 * k["log"] * U * math.log(S) + U * np.abs(lpd).astype(np.float64))
    mean = l.sum(axis=1) / LD(S)
    dev = l - mean[:, None]
    m2 = (dev * dev).sum(axis=1)
    bmean = bl.mean(axis=1) + (D + 1.0) * U * la.max(axis=1)
    e = bl + bmean[:, None] + U * np.abs(dev).astype(np.float64)
    bm2 = (2.0 * np.abs(dev).astype(np.float64) * e + e * e).sum(axis=1) + (D + 4.0) * U * m2.astype(np.float64)
    ref = dict(l=l.astype(np.float64), lpd=lpd.astype(np.float64), lmean=mean.astype(np.float64), lm2=m2.astype(np.float64))
    bound = dict(l=bl, lpd=blpd, lmean=bmean, lm2=bm2)
    if not link:
        rf = r.astype(np.float64)
        pv = _phi_ld(rf)
        ref["pit"] = (pv.sum(axis=1) / LD(S)).astype(np.float64)
        bound["pit"] = (sc.phi_pdf(rf) * (er + 2.0 * U * ra) + sc.ERFC_C * U).mean(axis=1) + (D + 1.0) * U
    return ref, bound


def from_z(z, bz, sigma=None, key=0, probs=(), y=None, row_scale=None, link=0, first_row=0, figures=None):
    """The read-out of the matrix z [rows x S] (known to within bz) with sigma [S] per pooled draw (link 0).  Row i of the matrix is row first_row + i
    of the call (the counter of the noise).  Returns (ref, bound): quantiles [Q x rows] where probs are given, the scores where y is; ref also z and
    y_rep (float64)."""
    z = np.asarray(z, dtype=np.float64)
    rows, S = z.shape
    ref, bound = dict(z=z), dict(z=bz)
    sd = None
    if not link:
        rs = np.ones(rows) if row_scale is None else np.asarray(row_scale, dtype=np.float64)
        sd = rs[:, None] * np.asarray(sigma, dtype=np.float64)[None, :]          # fl(sigma * row_scale) in double, as the device forms it
    if len(probs):
        assert not link
        e, be = noise(key, np.arange(first_row, first_row + rows), np.arange(S), figures)
        yrep = z.astype(LD) + sd.astype(LD) * e
        by = bz + sd * be + U * (np.abs(z) + 2.0 * sd * np.abs(e).astype(np.float64))
        ref["y_rep"], bound["y_rep"] = yrep.astype(np.float64), by
        ref["quantiles"] = qc.type7(yrep, probs).astype(np.float64)
        bound["quantiles"] = qc.bound(yrep.astype(np.float64), by, len(probs))
    if y is not None:
        r2, b2 = score(z, bz, y, sd, link, figures)
        ref.update(r2)
        bound.update(b2)
    return ref, bound


def model(parts, key=0, probs=(), y=None, row_scale=None, link=0, first_row=0, offset=None, dense=None, ell_index=None, ell_value=None, figures=None):
    """`parts`: per pooled sampler, in pooling order, dict(bart [rows x draws], sigma [draws] (link 0), dense_coef, ell_coef); the row side of the
    linear parts as quantile_cases.model takes it.  from_z of the pooled z."""
    z, bz = pooled_z(parts, offset, dense, ell_index, ell_value)
    sigma = None if link else np.concatenate([np.asarray(p["sigma"], dtype=np.float64) for p in parts])
    return from_z(z, bz, sigma, key, probs, y, row_scale, link, first_row, figures)


OUTPUTS = ("quantiles", "lpd", "lmean", "lm2", "pit")


def assert_ppd(got, ref, bound, what, report=print):
    """A Sampler.predict_ppd result against model(): every entry of every output the model holds within BOUND_FACTOR x its bound, and no output the
    model does not hold.  The ratios are printed before they are asserted."""
    ratios = {}
    for key in OUTPUTS:
        if key in ref:
            assert got[key] is not None and got[key].shape == ref[key].shape, (what, key)
            ratios[key] = bound_ratio(got[key], ref[key], bound[key])
        else:
            assert got[key] is None or got[key].size == 0, (what, key, "formed though not asked for")
    info = got["info"]
    report(f"predict_ppd {what}: route {info['route']}, {info['chunks']} chunk(s) of {info['rows_per_chunk']} rows, {info['rows_per_sort']} row(s) per "
           f"workgroup at {info['padded_draws']} padded draws, max |device - model| / bound: " + ", ".join(f"{k} {r:.3g}" for k, r in ratios.items()))
    for key, r in ratios.items():
        assert r <= BOUND_FACTOR, f"{what}: {key} is {r:.3g} x the derived bound (allowed: {BOUND_FACTOR:g})"
    return ratios


def device_bytes_formula(P, rows, nodes, S, T, offset, M, E, q, C, Q, link, row_scale, y, lpd, moments, pit):
    """the device memory of one call (every allocation at least 16 bytes).  The only rows-times-draws term is the chunk's: 8 C S."""
    sizes = [2 * P * rows, 24 * nodes, 8 * S * T, 16 * S, 8 * C * S]          # binned rows, nodes, tree starts, scales, values
    if offset:
        sizes.append(8 * rows)
    if M:
        sizes += [8 * rows * M, 8 * S * M]
    if E:
        sizes += [4 * rows * E, 8 * rows * E, 8 * S * q]
    if Q:
        sizes += [8 * Q, 8 * Q * rows]
    if not link:
        sizes += [8 * S] + ([8 * rows] if row_scale else [])
    if y:
        sizes += [8 * rows] * (1 + bool(lpd) + 2 * bool(moments) + bool(pit))
    return sum(max(16, t) for t in sizes)
