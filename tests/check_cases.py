"""s4b_predict_check (stan4bart_amd/csrc/readout_check.inc over dev_readout.inc, dev_quantile.inc, dev_groups.inc, readout_spread.inc and philox.hpp:
k_predict_values unchanged, k_check_reduce, k_check_fold, k_check_finish, k_level_rows and k_row_quantiles unchanged) — the model, the bounds and the
inputs shared by tests/test_predict_check.py (CPU) and tests/test_gpu_predict_check.py (GPU).

The reference is numpy in long double on the FULL [rows x pooled draws] replicate matrix x, at shapes where the matrix is small:
  z, bz    the value kernel's z with its bound (quantile_cases.model / ppd_cases.pooled_z);
  link 0   x = z + sd e, sd = fl(sigma[k] row_scale[i]) in double, e = ppd_cases.noise (its Philox, its noise model and its bound of e), and
           bx = bz + sd be + u (|z| + 2 sd |e|): ppd_cases' bound of y_rep;
  link 1   x = 1 where u <= Phi(z) else 0, u = latent_par_cases.u53 of the first two words of the same block, Phi = summary_cases.phi_cdf with
           bPhi = phi(z) (bz + 2 u |z|) + ERFC_C u (ppd_cases' bound of Phi); an element with |u - Phi| <= BOUND_FACTOR bPhi is AMBIGUOUS, every other
           replicate is exact on both sides (bx = 0);
and per draw, with W = the weights added in row order IN DOUBLE (group_cases.host_weight)
    mean, sd, min, max, share_above     spread_cases.model of x (the same slab arithmetic: its bounds hold unchanged; the slab's M2 is formed as
                                        s2 - (s1 / W_s) s1 instead of s2 - s1^2 / W_s, the same count of roundings),
    m3 = sum_i w_i (x_i - mean)^3 / W,
    link 0: disc_rep = sum_i w_i e^2 / W,  disc_obs = sum_i w_i ((y_i - z) / sd)^2 / W;   link 1: disc = -2 sum_i w_i log Phi(+-z) / W,
the matrix D [(7 + T) x S] = mean, sd, m3, min, max, share_above[0 .. T), disc_rep, disc_obs, over the draws summary_cases.summarise and
quantile_cases.type7 / bound as spread_cases uses them, and observed [5 + T] = the same model at x = y (one column).  y is exact on both sides; what
stands in as its bx is the REFERENCE's own rounding, 8 eps |y| with eps the long double's: where the answer is exactly 0 on the device (one row of
weight w: sd = m3 = 0) the reference's w y / w is not exactly y, and a bound of 0 would hold the device against that.

BOUNDS (u = 2^-53; no measured constant; every comparison allows readout_cases.BOUND_FACTOR x the bound).  spread_cases' notation: B = SLAB,
slabs = ceil(n / B), adds = min(n, B) + slabs + 1, cnt = slabs (2 adds + 5), rng = max x - min x + 2 max bx over ALL rows, amax = max |x| + max bx;
every difference the device forms is at most rng, every value at most amax, so |M2| <= W rng^2 and |M3| <= W rng^3 at every stage.
  eD   = (2 cnt + 1) u rng + 2 (slabs + 1) u amax          the rounding part of delta = mean_b - mean_a (spread_cases' second-moment paragraph)
  RM2  = ((4 cnt + 7 adds + 2 slabs + 16) rng^2 + 4 (slabs + 1) amax rng) u W          spread_cases' rounding(M2): covers every partial and running M2
Third moment, slab form M3_s = (s3 - 3 d s2) + 2 d^2 s1, d = s1 / W_s.  s3 = fold of w d_i^3: a subtraction, three products and at most min(n, B)
additions per term: (adds + 4) u W_s rng^3; s2 (adds + 3) u W_s rng^2; s1 (adds + 2) u W_s rng; d = s1 / W_s adds W_s' adds u and the division:
(2 adds + 3) u rng.  3 d s2 (at most 3 W_s rng^3) carries d's, s2's and three roundings: (3 adds + 9) u relative; 2 d^2 s1 (at most 2 W_s rng^3)
twice d's, s1's and two roundings: (5 adds + 10) u relative; the two additions at most u (1 + 3 + 2) W_s rng^3 each.  Together
    slab(M3) = ((adds + 4) + 3 (3 adds + 9) + 2 (5 adds + 10) + 12) u W_s rng^3 = (20 adds + 63) u W_s rng^3.
Pebay's update adds A = delta^3 W_a W_b (W_a - W_b) / W^2 and Bt = 3 delta (W_a M2_b - W_b M2_a) / W.  |A| <= rng^3 W_b: delta moves it by
3 rng^2 eD W_b, the difference of the weights by (adds + 1) u W_b rng^3, W_a, W_b and W^2 by 4 adds u, the eight operations by 8 u:
(5 adds + 9) u W_b rng^3 + 3 rng^2 eD W_b.  |Bt| <= 6 W_b rng^3: delta moves it by 6 rng^2 eD W_b, the weights and the six operations by
(3 adds + 6) u relative, the errors of M2_b and M2_a by 3 rng (err M2_b + (W_b / W) err M2_a) <= 3 rng RM2 per step at most (slabs steps).
The three additions of a step carry u W rng^3 each.  Summed over the slabs (sum of W_b <= W):
    rounding(M3) = (43 adds + 108 + 3 slabs) u W rng^3 + 9 W rng^2 eD + 3 slabs rng RM2
and the inputs move M3 by at most sum_i w_i (3 a_i^2 e_i + 3 a_i e_i^2 + e_i^3), a_i = |x_i - mean|, e_i = bx_i + w' bx / W:
    bound(m3) = (inputs + rounding(M3)) / W + u |m3|.
The terms amax appear only through eD and RM2, multiplied by rng^2: that is what the shift buys; the raw form sum w x^3 - 3 mean sum w x^2 + 2 mean^3 W
carries u W amax^3.
Discrepancies.  A slab's fold passes at most min(n, B) additions, the slabs slabs more, then a product or none and a division: (adds + 4) u
relative on sums of terms of one sign (a term itself rounds twice), beside what the inputs move:
    link 0   bound(disc_rep) = sum_i w_i (2 |e| be + be^2) / W + (adds + 4) u disc_rep
             bound(disc_obs) = sum_i w_i (2 |r| er + er^2) / W + (adds + 4) u disc_obs,   er = (bz + u |y - z|) / sd + u |r|   (ppd_cases' r)
    link 1   bound(disc) = 2 sum_i w_i (bl + u |l|) / W + (adds + 4) u |disc|,   bl ppd_cases' bound of l = log Phi(+-z) at the sign taken.
Link 0: a replicate within BOUND_FACTOR x bx of a finite threshold is AMBIGUOUS (spread_cases' rule).  The cases take their finite thresholds from
group_cases.midway over the reference replicate (spread_cases.thresholds_for) and their noise keys so that NO element is ambiguous; the tests
assert that and never skip over it.

DEVICE MEMORY of one call (device_bytes_formula): the value kernel's inputs and the chunk's scratch 8 C S, and beyond them, with
R = 8 + (T + 1 where T > 0) and M = 7 + T: y 8 n, the weights 8 n (if given), sigma 8 S and row_scale 8 n (link 0; if given), the thresholds 8 T, the
slab partials 8 ceil(C / SLAB) R S, the totals 8 R S, the matrix 8 M S, the M + 1 row marks, M unit weights, M doubles per summary asked for, the
probs and 8 Q M.  Nothing grows with n x S beyond the chunk."""
import numpy as np

import group_cases as gc
import latent_par_cases as lp
import ppd_cases as ppd
import quantile_cases as qc
import spread_cases as sp
import summary_cases as sc
from readout_cases import BOUND_FACTOR, U, bound_ratio  # noqa: F401

LD = np.longdouble
LD_EPS = float(np.finfo(LD).eps)
SLAB = sp.SLAB
THRESHOLDS_MAX = sp.THRESHOLDS_MAX
FLOATS = ("draws", "mean", "m2", "quantiles", "observed")
_M32 = np.uint64(0xFFFFFFFF)


def names(T):
    return ["mean", "sd", "m3", "min", "max"] + [f"share_above[{j}]" for j in range(T)] + ["disc_rep", "disc_obs"]


def uniform(key, rows, draws):
    """u [len(rows) x len(draws)] in double: philox_uniform of philox.hpp — u53 of the first two words of ppd_cases.noise's block."""
    i = np.asarray(rows, dtype=np.uint64)[:, None]
    d = np.asarray(draws, dtype=np.uint64)[None, :]
    r = lp.philox4x32_10(i & _M32, i >> np.uint64(32), d, ppd.PPD_TAG, int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF)
    return lp.u53(r[0], r[1])


def replicate(z, bz, sigma=None, key=0, row_scale=None, link=0, first_row=0):
    """The replicate matrix of z [rows x S] (known to within bz): dict(x (long double), bx, ambiguous (link 1: the elements whose uniform lies within
    BOUND_FACTOR x the bound of Phi(z)), e, be, sd (link 0), l1, bl1, l0, bl0 (link 1: log Phi(z), log Phi(-z) and their bounds))."""
    z = np.asarray(z, dtype=np.float64)
    bz = np.broadcast_to(np.asarray(bz, dtype=np.float64), z.shape)
    n, S = z.shape
    rows, draws = np.arange(first_row, first_row + n), np.arange(S)
    if link:
        u = uniform(key, rows, draws)
        Phi = sc.phi_cdf(z)
        bPhi = sc.phi_pdf(z) * (bz + 2.0 * U * np.abs(z)) + sc.ERFC_C * U
        x = np.where(u <= Phi, 1.0, 0.0).astype(LD)
        r1, b1 = ppd.score(z, bz, np.ones(n), None, 1)
        r0, b0 = ppd.score(z, bz, np.zeros(n), None, 1)
        return dict(x=x, bx=np.zeros(z.shape), ambiguous=int((np.abs(u - Phi) <= BOUND_FACTOR * bPhi).sum()), l1=r1["l"], bl1=b1["l"] + U * np.abs(r1["l"]),
                    l0=r0["l"], bl0=b0["l"] + U * np.abs(r0["l"]))
    rs = np.ones(n) if row_scale is None else np.asarray(row_scale, dtype=np.float64)
    sd = rs[:, None] * np.asarray(sigma, dtype=np.float64)[None, :]          # fl(sigma * row_scale) in double, as the device forms it
    e, be = ppd.noise(key, rows, draws)
    x = z.astype(LD) + sd.astype(LD) * e
    bx = bz + sd * be + U * (np.abs(z) + 2.0 * sd * np.abs(e).astype(np.float64))
    return dict(x=x, bx=bx, ambiguous=0, e=e, be=be, sd=sd)


def third_moment(x, bx, weights=None):
    """(m3 [S] long double, bound) of the columns of x by the module docstring."""
    x = np.asarray(x, dtype=LD)
    n, S = x.shape
    bx = np.broadcast_to(np.asarray(bx, dtype=np.float64), x.shape)
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    W = gc.host_weight(w)
    wl = w.astype(LD)[:, None]
    slabs = -(-n // SLAB)
    adds = min(n, SLAB) + slabs + 1
    cnt = slabs * (2 * adds + 5)
    xf = x.astype(np.float64)
    bmax = bx.max(axis=0)
    rng = (xf.max(axis=0) - xf.min(axis=0)) + 2.0 * bmax
    amax = np.abs(xf).max(axis=0) + bmax
    mean = (wl * x).sum(axis=0) / LD(W)
    dev = x - mean[None, :]
    m3 = (wl * dev * dev * dev).sum(axis=0) / LD(W)
    eD = (2 * cnt + 1) * U * rng + 2.0 * (slabs + 1) * U * amax
    RM2 = ((4 * cnt + 7 * adds + 2 * slabs + 16) * rng * rng + 4.0 * (slabs + 1) * amax * rng) * U * W
    rounding = (43 * adds + 108 + 3 * slabs) * U * W * rng ** 3 + 9.0 * W * rng * rng * eD + 3.0 * slabs * rng * RM2
    a = np.abs(dev).astype(np.float64)
    e = bx + ((w[:, None] * bx).sum(axis=0) / W)[None, :]
    inputs = (w[:, None] * (3.0 * a * a * e + 3.0 * a * e * e + e ** 3)).sum(axis=0)
    return m3, (inputs + rounding) / W + U * np.abs(m3).astype(np.float64)


def statistics(x, bx, weights=None, thresholds=()):
    """(D, bD) [(5 + T) x S]: mean, sd, m3, min, max, share_above of the columns of x; also spread_cases' ref (weight, zero_slabs, ambiguous)."""
    th = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    T = len(th)
    ref, bd = sp.model(x, bx, weights, th, ())
    m3, bm3 = third_moment(x, bx, weights)
    pick = [0, 1, None, 2, 3] + list(range(4, 4 + T))
    S = np.shape(x)[1]
    D, bD = np.zeros((5 + T, S), dtype=LD), np.zeros((5 + T, S))
    for m, src in enumerate(pick):
        D[m], bD[m] = (m3, bm3) if src is None else (ref["draws"][src], bd["draws"][src])
    return D, bD, ref


def model(z, bz, y, sigma=None, key=0, weights=None, thresholds=(), probs=(), row_scale=None, link=0, first_row=0):
    """Returns (ref, bound): dicts with draws [(7 + T) x S], mean, m2 [7 + T], quantiles [Q x (7 + T)], observed [5 + T]; ref also weight,
    zero_slabs, thresholds, x (the replicate, float64) and `ambiguous`, the number of elements the device may replicate or bin otherwise."""
    z = np.asarray(z, dtype=np.float64)
    n, S = z.shape
    y = np.asarray(y, dtype=np.float64)
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    th = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    T = len(th)
    assert not (link and T), "the call is refused: thresholds under link 1"
    rep = replicate(z, bz, sigma, key, row_scale, link, first_row)
    x, bx = rep["x"], rep["bx"]
    head, bhead, spref = statistics(x, bx, weights, th)
    W = spref["weight"]
    slabs = -(-n // SLAB)
    adds = min(n, SLAB) + slabs + 1
    wl = w.astype(LD)[:, None]
    wc = w[:, None]
    if link:
        one_rep, one_obs = np.asarray(x, dtype=np.float64) > 0.0, np.broadcast_to((y > 0.0)[:, None], z.shape)
        disc, bdisc = [], []
        for one in (one_rep, one_obs):
            l, bl = np.where(one, rep["l1"], rep["l0"]), np.where(one, rep["bl1"], rep["bl0"])
            d = LD(-2.0) * (wl * l.astype(LD)).sum(axis=0) / LD(W)
            disc.append(d)
            bdisc.append(2.0 * (wc * bl).sum(axis=0) / W + (adds + 4) * U * np.abs(d).astype(np.float64))
    else:
        e, be, sd = rep["e"], rep["be"], rep["sd"]
        ea = np.abs(e).astype(np.float64)
        r = (y.astype(LD)[:, None] - z.astype(LD)) / sd.astype(LD)
        ra = np.abs(r).astype(np.float64)
        er = (np.broadcast_to(bz, z.shape) + U * np.abs(y[:, None] - z)) / sd + U * ra
        disc = [(wl * e * e).sum(axis=0) / LD(W), (wl * r * r).sum(axis=0) / LD(W)]
        bdisc = [(wc * (2.0 * ea * be + be * be)).sum(axis=0) / W + (adds + 4) * U * disc[0].astype(np.float64),
                 (wc * (2.0 * ra * er + er * er)).sum(axis=0) / W + (adds + 4) * U * disc[1].astype(np.float64)]
    D = np.vstack([head, disc[0][None, :], disc[1][None, :]])
    bD = np.vstack([bhead, bdisc[0][None, :], bdisc[1][None, :]])
    obs, bobs, _ = statistics(y[:, None].astype(LD), 8.0 * LD_EPS * np.abs(y)[:, None], weights, th)          # (module docstring: the reference's own roundings)
    ref = dict(draws=D, weight=W, zero_slabs=spref["zero_slabs"], ambiguous=rep["ambiguous"] + spref["ambiguous"], thresholds=th,
               x=np.asarray(x, dtype=np.float64), bx=bx, observed=obs[:, 0])
    bound = dict(draws=bD, observed=bobs[:, 0])
    r_, b_ = sc.summarise(D, bD)
    ref["mean"], ref["m2"], bound["mean"], bound["m2"] = r_["mean"], r_["m2"], b_["mean"], b_["m2"]
    if len(probs):
        ref["quantiles"] = qc.type7(D, probs).astype(np.float64)
        bound["quantiles"] = qc.bound(D.astype(np.float64), bD, len(probs))
    return ref, bound


def _moments(xs, ws):
    """One column by the stated order in double: (W, mean, M2, M3, min, max) — the slab sums, the slab partials, the pairwise update."""
    Wa = mean = M2 = M3 = 0.0
    mn, mx = np.inf, -np.inf
    for r0 in range(0, len(xs), SLAB):
        c, Ws, s1, s2, s3 = float(xs[r0]), 0.0, 0.0, 0.0, 0.0
        for xi, wi in zip(xs[r0:r0 + SLAB], ws[r0:r0 + SLAB]):
            xi, wi = float(xi), float(wi)
            d = xi - c
            wd = wi * d
            wdd = wd * d
            Ws, s1, s2, s3 = Ws + wi, s1 + wd, s2 + wdd, s3 + wdd * d
            if wi > 0.0:
                mn, mx = min(mn, xi), max(mx, xi)
        if not Ws > 0.0:
            continue
        d = s1 / Ws
        ms, M2s, M3s = c + d, max(0.0, s2 - d * s1), (s3 - 3.0 * d * s2) + 2.0 * d * d * s1
        if not Wa > 0.0:
            Wa, mean, M2, M3 = Ws, ms, M2s, M3s
            continue
        delta, Wn = ms - mean, Wa + Ws
        M3 = M3 + M3s + delta * delta * delta * Wa * Ws * (Wa - Ws) / (Wn * Wn) + 3.0 * delta * (Wa * M2s - Ws * M2) / Wn
        M2 = M2 + M2s + delta * delta * Wa * Ws / Wn
        mean = mean + delta * Ws / Wn
        Wa = Wn
    return Wa, mean, M2, M3, mn, mx


def _fold(terms):
    """Left folds per slab from +0, then over the slabs."""
    tot = 0.0
    for r0 in range(0, len(terms), SLAB):
        s = 0.0
        for t in terms[r0:r0 + SLAB]:
            s = s + float(t)
        tot = tot + s
    return tot


def device_order(x, weights=None, thresholds=(), disc_terms=None, link=0):
    """The statement of include/stan4bart_amd.h carried out literally in double, one draw at a time, on the replicate matrix x [rows x S] (float64):
    D [(5 + T) x S], or [(7 + T) x S] with `disc_terms` = (rep, obs), the two [rows x S] matrices of the UNWEIGHTED terms (e e and r r, or
    log Phi(+-z)).  Without fused multiply-adds, so it agrees with a device to rounding only; the CPU tests hold it against model() within the
    bounds, which checks that the bounds cover the stated order."""
    x = np.asarray(x, dtype=np.float64)
    n, S = x.shape
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    th = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    T = len(th)
    W = gc.host_weight(w)
    D = np.zeros((5 + T + (2 if disc_terms is not None else 0), S))
    for k in range(S):
        _, mean, M2, M3, mn, mx = _moments(x[:, k], w)
        D[0, k], D[1, k], D[2, k], D[3, k], D[4, k] = mean, np.sqrt(M2 / W), M3 / W, mn, mx
        cw = np.zeros(T + 1)
        for r0 in range(0, n, SLAB):
            pw = np.zeros(T + 1)
            for xi, wi in zip(x[r0:r0 + SLAB, k], w[r0:r0 + SLAB]):
                pw[int((xi > th).sum())] += wi
            cw = cw + pw
        aw = 0.0
        for b in range(T, 0, -1):
            aw = aw + cw[b]
            D[5 + b - 1, k] = aw / W
        if disc_terms is not None:
            for j, t in enumerate(disc_terms):
                tot = _fold(w * np.asarray(t, dtype=np.float64)[:, k])
                D[5 + T + j, k] = (-2.0 * tot if link else tot) / W
    return D


def raw_third_moment(xs, ws=None):
    """What the shift avoids: sum w x^3 - 3 mean sum w x^2 + 2 mean^3 W over W, in double."""
    xs = np.asarray(xs, dtype=np.float64)
    ws = np.ones(len(xs)) if ws is None else np.asarray(ws, dtype=np.float64)
    W = gc.host_weight(ws)
    s1 = s2 = s3 = 0.0
    for xi, wi in zip(xs, ws):
        s1, s2, s3 = s1 + wi * xi, s2 + wi * xi * xi, s3 + wi * xi * xi * xi
    m = s1 / W
    return (s3 - 3.0 * m * s2 + 2.0 * m * m * m * W) / W


def brute_force(x, weights=None, thresholds=()):
    """Plain numpy, double precision: what a user would write over the replicate matrix.  [(5 + T) x S]."""
    x = np.asarray(x, dtype=np.float64)
    n, S = x.shape
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    T = len(thresholds)
    D = np.zeros((5 + T, S))
    for k in range(S):
        m = np.average(x[:, k], weights=w)
        D[0, k] = m
        D[1, k] = np.sqrt(np.average((x[:, k] - m) ** 2, weights=w))
        D[2, k] = np.average((x[:, k] - m) ** 3, weights=w)
        D[3, k], D[4, k] = x[w > 0.0, k].min(), x[w > 0.0, k].max()
        for j, t in enumerate(thresholds):
            D[5 + j, k] = w[x[:, k] > t].sum() / w.sum()
    return D


def p_values(D, observed, T):
    """The posterior predictive p-values as Stan4bartFit.pp_check forms them: per statistic of `observed` the share of draws with D >= observed, and
    the share with disc_rep >= disc_obs."""
    D = np.asarray(D, dtype=np.float64)
    return np.array([np.mean(D[m] >= observed[m]) for m in range(5 + T)]), float(np.mean(D[5 + T] >= D[6 + T]))


def assert_check(got, ref, bound, what, report=print, weighted=False):
    """A Sampler.predict_check result against model(): every floating output within BOUND_FACTOR x its bound, none left out; W exactly; without
    weights share_above exactly (its bound is 0).  The ratios are printed before they are asserted."""
    info = got["info"]
    T = len(ref["thresholds"])
    assert ref["ambiguous"] == 0, f"{what}: {ref['ambiguous']} element(s) lie within their bound of a threshold or of Phi(z): choose another key or other thresholds"
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
    parts = {"d.mean": slice(0, 1), "d.sd": slice(1, 2), "d.m3": slice(2, 3), "d.minmax": slice(3, 5), "d.disc_rep": slice(5 + T, 6 + T),
             "d.disc_obs": slice(6 + T, 7 + T)}
    if T:
        parts["d.share"] = slice(5, 5 + T)
    for key, rows in parts.items():
        ratios[key] = bound_ratio(g[rows], r[rows], b[rows])
    report(f"predict_check {what}: route {info['route']}, {info['chunks']} chunk(s) of {info['rows_per_chunk']} rows, T = {T}, {info['draws']} draws, "
           f"{info['zero_slabs']} slab(s) without weight; max |device - model| / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    for key, v in ratios.items():
        assert v <= BOUND_FACTOR, f"{what}: {key} is {v:.3g} x the derived bound (allowed: {BOUND_FACTOR:g})"
    if T and not weighted:
        assert np.array_equal(g[5:5 + T], r[5:5 + T].astype(np.float64)), f"{what}: share_above differs from the model's exact count / n"
    return ratios


def device_bytes_formula(value_bytes, rows, S, T, C, link=0, weights=False, row_scale=False, mean=True, m2=True, Q=0):
    """the device memory of one call (every allocation at least 16 bytes).  `value_bytes`: what the value kernel's inputs and the
    chunk's scratch take (quantile_cases.device_bytes_formula without outputs).  No term grows with rows x S beyond the chunk."""
    R, M = 8 + (T + 1 if T else 0), 7 + T
    sizes = [8 * rows, 8 * -(-C // SLAB) * R * S, 8 * R * S, 8 * M * S, 8 * (M + 1), 8 * M]
    sizes += [8 * rows] * bool(weights) + [8 * T] * bool(T) + [8 * M] * (int(bool(mean)) + int(bool(m2)))
    if not link:
        sizes += [8 * S] + [8 * rows] * bool(row_scale)
    if Q:
        sizes += [8 * Q, 8 * Q * M]
    return value_bytes + sum(max(16, t) for t in sizes)
