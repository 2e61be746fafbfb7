"""s4b_predict_loo (stan4bart_amd/csrc/dev_loo.inc: k_predict_values<staged / global> unchanged, k_loo_rows) — the model, the bound and
the cases shared by tests/test_predict_loo.py (CPU) and tests/test_gpu_predict_loo.py (GPU).

THE MODEL is numpy in long double on the FULL [rows x pooled draws] matrix: l and its element bound bl are ppd_cases.score's / pooled_z's (predict_ppd's
log-likelihood, link 0 or 1); `psis` then applies the definition of include/stan4bart_amd.h literally — sort lr = -l, lw = lr - max, the tail of M, the
generalised-Pareto fit over the grid of G = 30 + floor(sqrt M) points, khat, the smoothed tail, the four outputs.

THE BOUND of an entry has two parts; the tests allow readout_cases.BOUND_FACTOR x their sum.
  derived   u = 2^-53, k_f the error of library function f in ulps (latent_par_cases.DEVICE, assumed as in ppd_cases), D = ppd_cases.tree_depth(S) + 2
            the additions on the longest path of a row sum of k_loo_rows (the lanes, the butterfly, the waves of the row, and the one term that stands
            for the S - M draws outside the tail).  A log-sum-exp m + log(sum_j exp(a_j - m)) of EXACT arguments: the differences round
            (u sum_j t_j |a_j - m| / sum t), exp 2 k_exp u, the sum D u, the logarithm 2 k_log u |log sum|, the last sum u |m + log sum| (`_lse_arith`).
              elpd_loo  both log-sum-exps and the difference u |elpd|; the arguments themselves carry u (|lw| + |lr|) outside the tail (the kernel
                        takes -mx for lw + l there) and the rounding of lw' - lr inside it: 2 u max_j (|lw'_j| + |lr_j|)
              lpd       ppd_cases' lpd argument: max_k bl (log-sum-exp is 1-Lipschitz), the log-sum-exp, log S: 2 k_log u log S, u |lpd|
              ess       sB^2 / sC relative: twice the sum of exp(lw' - mB) ((D + 2 k_exp) u + the rounded arguments 2 u max |lw'|, weighted), the
                        sum of squares the same twice plus a square each (u), a product and a quotient (2 u)
              pareto_k  the last four operations: 4 u |khat| + 4 u
  measured  the map l -> (khat, smoothed tail) has no usable closed Lipschitz constant.  For it the MODEL'S OWN SENSITIVITY is taken: the long-double
            model is evaluated on l + s bl under 16 seeded sign patterns s, each also moving the tail values x_j by s' ((2 k_exp u + u |lw|) e^lw +
            2 k_exp u ec + u x_j) (what the device's exponentials and the difference may add before the fit sees them) and kappa_g, L_g and k0 by the
            error of their sums at the kernel's reduction depth (`fit_depth`) and of their library calls (`gpd_fit`), and once more in float64 (the
            rounding of the rest of the fit's arithmetic: the grid, the weights, theta^, the smoothed tail).  The largest deviation from the long-double model over
            these 17 runs is the measured part.  Measured against the reference, never against the device.
Long double and double underflow at different arguments (exp below -745 against -11355), so a reference in long double says nothing about a row whose
ratios underflow against the largest one in double: the cases keep the likelihoods of a row within a few hundred of each other, and the underflow is a
planted row of its own (it may be left out, see next).
A row is LEFT OUT of the numeric comparison only where these runs disagree on the branch (smoothed against +inf); `model` asserts that at most 2 % of a
case's rows are, and the GPU tests still ask for a finite elpd_loo and a finite-or-+inf pareto_k there."""
import math

import numpy as np

import latent_par_cases as lp
import ppd_cases as pp
from readout_cases import BOUND_FACTOR, U, bound_ratio  # noqa: F401

LD = np.longdouble
OUTPUTS = ("elpd_loo", "pareto_k", "lpd", "ess")
TAIL_MAX = 1024
DRAWS_MAX = 16384
PATTERNS = 16
LEFT_OUT_MAX = 0.02
K_LOG1P = 1.0          # log1p and expm1 in ulps: ASSUMED, as latent_par_cases.DEVICE's figures are (the HIP programming guide's table states 1)


def tail_len(S):
    """min(ceil(S / 5), ceil(3 sqrt S)), the second as the smallest m with m m >= 9 S: integers only."""
    S = int(S)
    m = math.isqrt(9 * S)
    if m * m < 9 * S:
        m += 1
    return min(-(-S // 5), m)


def tail_len_r_eff(S, r_eff):
    """The fit method's host rule for r_eff != 1."""
    return int(math.ceil(min(S / 5.0, 3.0 * math.sqrt(S / float(r_eff)))))


def fit_depth(N):
    """The additions on the longest path of the two sums of the fit in k_loo_rows: kappa_g (a lane runs over the N tail values with four partial sums,
    then folds them) and k0 (lane-strided, then the butterfly)."""
    return -(-int(N) // 4) + 2, -(-int(N) // 64) + 6


def gpd_fit(x, dtype=LD, jitter=None):
    """(khat, sigma) of the generalised-Pareto fit to the ascending tail values x [rows x N] (step 3 of the definition); not finite where it fails.
    `jitter`: a Generator whose signs move kappa_g, L_g and k0 by the arithmetic error of the kernel's sums and library calls (module docstring)."""
    x = np.asarray(x, dtype=dtype)
    rows, N = x.shape
    G = 30 + math.isqrt(N)
    g = np.arange(1, G + 1).astype(dtype)
    k, (dk, d0) = lp.DEVICE, fit_depth(N)
    sign = (lambda shape: jitter.choice([-1.0, 1.0], size=shape).astype(dtype) * dtype(U)) if jitter is not None else None
    with np.errstate(all="ignore"):
        xs = x[:, int(math.floor(N / 4.0 + 0.5)) - 1]
        theta = dtype(1) / x[:, -1:] + (dtype(1) - np.sqrt(dtype(G) / (g - dtype(0.5))))[None, :] / (dtype(3) * xs[:, None])
        kap = np.empty((rows, G), dtype=dtype)
        for a in range(0, rows, 16):          # [16 x G x N] at a time
            t = np.log1p(-theta[a:a + 16, :, None] * x[a:a + 16, None, :])
            kap[a:a + 16] = t.mean(axis=2)
            if sign is not None:          # log1p K_LOG1P ulps and the rounded product per term, the sum, the quotient
                kap[a:a + 16] += sign((len(t), G)) * (dk + 2.0 * K_LOG1P + 2.0) * np.abs(t).mean(axis=2)
        L = dtype(N) * (np.log(-theta / kap) - kap - dtype(1))
        if sign is not None:          # the quotient, the logarithm, two differences, the product
            L = L + sign(L.shape) * dtype(N) * ((1.0 + 2.0 * k["log"]) * (1.0 + np.abs(np.log(-theta / kap))) + 2.0 * (np.abs(kap) + 1.0)) + sign(L.shape) * np.abs(L)
        e = np.exp(L - L.max(axis=1, keepdims=True))
        w = e / e.sum(axis=1, keepdims=True)
        th = (theta * w).sum(axis=1)
        t0 = np.log1p(-th[:, None] * x)
        k0 = t0.mean(axis=1)
        if sign is not None:
            k0 = k0 + sign(k0.shape) * (d0 + 2.0 * K_LOG1P + 2.0) * np.abs(t0).mean(axis=1)
        sigma = -k0 / th
        khat = k0 * dtype(N) / dtype(N + 10) + dtype(5) / dtype(N + 10)
    return khat, sigma


def _lse(a):
    m = a.max(axis=1)
    with np.errstate(all="ignore"):
        return m + np.log(np.exp(a - m[:, None]).sum(axis=1))


def psis(l, M, dtype=LD, jitter=None):
    """The definition applied to the log-likelihoods l [rows x S] with tail length M, in `dtype`.  `jitter`: None or a Generator whose signs move
    the tail values x_j by their arithmetic error before the fit (module docstring).  Returns dict(elpd_loo, pareto_k, lpd, ess [rows] in dtype,
    smoothed [rows] bool, lr, lwp [rows x S]: the sorted log ratios and the weights used)."""
    l = np.asarray(l).astype(dtype)
    rows, S = l.shape
    lr = np.sort(-l, axis=1)
    lw = lr - lr[:, -1:]
    lwp = lw.copy()
    khat = np.full(rows, np.inf, dtype=dtype)
    smoothed = np.zeros(rows, dtype=bool)
    if M >= 5:
        assert M <= S - 1
        idx = np.nonzero(lw[:, -1] - lw[:, S - M] >= dtype(2.0 ** -52) / dtype(100))[0]
        if len(idx):
            t = lw[idx, S - M:]
            with np.errstate(all="ignore"):
                ec = np.exp(lw[idx, S - M - 1])[:, None]
                et = np.exp(t)
                x = et - ec
                if jitter is not None:
                    k = lp.DEVICE
                    s = jitter.choice([-1.0, 1.0], size=x.shape).astype(dtype)
                    x = x + s * dtype(U) * ((2.0 * k["exp"] + np.abs(t)) * et + 2.0 * k["exp"] * ec + np.abs(x))
                kh, sg = gpd_fit(x, dtype, jitter)
                ok = np.isfinite(kh) & np.isfinite(sg)
                p = (np.arange(M).astype(dtype) + dtype(0.5)) / dtype(M)
                sm = np.minimum(dtype(0), np.log(sg[:, None] * np.expm1(-kh[:, None] * np.log1p(-p)[None, :]) / kh[:, None] + ec))
            lwp[idx[ok], S - M:] = sm[ok]
            khat[idx[ok]] = kh[ok]
            smoothed[idx[ok]] = True
    with np.errstate(all="ignore"):
        elpd = _lse(lwp - lr) - _lse(lwp)
        lpd = _lse(-lr) - np.log(dtype(S))
        ess = np.exp(lwp).sum(axis=1) ** 2 / np.exp(dtype(2) * lwp).sum(axis=1)
    return dict(elpd_loo=elpd, pareto_k=khat, lpd=lpd, ess=ess, smoothed=smoothed, lr=lr, lwp=lwp)


def paired(l, M):
    """The PAIRED transliteration (loo's do_psis_i): the weights put back at their draws by argsort, elpd = logsumexp(l + lw) - logsumexp(lw).  What
    `psis` computes from the sorted row alone."""
    l = np.asarray(l).astype(LD)
    rows, S = l.shape
    out = np.empty(rows, dtype=LD)
    ks = np.empty(rows, dtype=LD)
    for i in range(rows):
        lw = -l[i] - np.max(-l[i])
        khat = LD(np.inf)
        if M >= 5:
            order = np.argsort(lw, kind="stable")
            tail_ids = order[S - M:]
            lw_tail = lw[tail_ids]
            if lw_tail[-1] - lw_tail[0] >= LD(2.0 ** -52) / LD(100):
                with np.errstate(all="ignore"):
                    ec = np.exp(lw[order[S - M - 1]])
                    kh, sg = gpd_fit((np.exp(lw_tail) - ec)[None, :])
                    if np.isfinite(kh[0]) and np.isfinite(sg[0]):
                        p = (np.arange(M).astype(LD) + LD(0.5)) / LD(M)
                        lw = lw.copy()
                        lw[tail_ids] = np.minimum(LD(0), np.log(sg[0] * np.expm1(-kh[0] * np.log1p(-p)) / kh[0] + ec))
                        khat = kh[0]
        with np.errstate(all="ignore"):
            out[i] = (_lse((l[i] + lw)[None, :]) - _lse(lw[None, :]))[0]
        ks[i] = khat
    return out, ks


def _lse_arith(a, D, k):
    """The arithmetic error of a log-sum-exp of exact arguments a [rows x S] (module docstring)."""
    a = np.asarray(a, dtype=LD)
    m = a.max(axis=1)
    with np.errstate(all="ignore"):
        t = np.exp(a - m[:, None])
        st = t.sum(axis=1)
        wd = (t * np.abs(np.where(t > 0, a - m[:, None], 0))).sum(axis=1) / st
        ls = np.log(st)
    return (U * wd + (D + 2.0 * k["exp"]) * U + 2.0 * k["log"] * U * np.abs(ls) + U * np.abs(m + ls)).astype(np.float64)


def from_l(l, bl, M, what="", left_out_max=LEFT_OUT_MAX, figures=None):
    """(ref, bound, compared) of the log-likelihoods l [rows x S] known to within bl: ref and bound hold OUTPUTS as float64 [rows], `compared` [rows]
    is False where the perturbed models disagree on the branch.  Asserts that at most left_out_max of the rows are left out."""
    k = lp.DEVICE if figures is None else figures
    l = np.asarray(l, dtype=np.float64)
    bl = np.broadcast_to(np.asarray(bl, dtype=np.float64), l.shape)
    rows, S = l.shape
    D = pp.tree_depth(S) + 2
    base = psis(l, M)
    runs = [psis(l, M, dtype=np.float64)]
    g = np.random.default_rng([20240, S, M, rows])
    for _ in range(PATTERNS):
        s = g.choice([-1.0, 1.0], size=l.shape)
        runs.append(psis(l.astype(LD) + (s * bl).astype(LD), M, jitter=g))
    compared = np.ones(rows, dtype=bool)
    dev = {key: np.zeros(rows) for key in OUTPUTS}
    for r in runs:
        compared &= r["smoothed"] == base["smoothed"]
        with np.errstate(all="ignore"):
            for key in OUTPUTS:
                d = np.abs(np.asarray(r[key], dtype=LD) - base[key]).astype(np.float64)
                dev[key] = np.maximum(dev[key], np.where(np.isfinite(d), d, 0.0))          # (inf - inf where both took the +inf branch)
    left = int((~compared).sum())
    assert left <= left_out_max * rows, f"{what}: {left} of {rows} rows change their branch under the perturbed models (allowed: 2 %)"
    lr, lwp = base["lr"], base["lwp"]
    ala = np.abs(lwp).astype(np.float64) + np.abs(lr).astype(np.float64)
    f = {key: np.asarray(base[key], dtype=np.float64) for key in OUTPUTS}
    arith = dict(
        elpd_loo=_lse_arith(lwp - lr, D, k) + _lse_arith(lwp, D, k) + 2.0 * U * ala.max(axis=1) + U * np.abs(f["elpd_loo"]),
        lpd=bl.max(axis=1) + _lse_arith(-lr, D, k) + 2.0 * k["log"] * U * math.log(S) + U * np.abs(f["lpd"]),
        ess=f["ess"] * (6.0 * (D + 2.0 * k["exp"]) * U + 8.0 * U * np.abs(lwp).astype(np.float64).max(axis=1) + 4.0 * U),
        pareto_k=np.where(base["smoothed"], 4.0 * U * np.abs(np.where(base["smoothed"], f["pareto_k"], 0.0)) + 4.0 * U, 0.0))
    dev["lpd"] = np.zeros(rows)          # (its input error is bl.max, derived)
    bound = {key: dev[key] + arith[key] for key in OUTPUTS}
    return f, bound, compared


def model(parts, y, M=None, row_scale=None, link=0, offset=None, dense=None, ell_index=None, ell_value=None, what="", figures=None):
    """`parts` as ppd_cases.model takes them.  from_l of the pooled log-likelihood; M None: the default tail length."""
    z, bz = pp.pooled_z(parts, offset, dense, ell_index, ell_value)
    return from_z(z, bz, None if link else np.concatenate([np.asarray(p["sigma"], dtype=np.float64) for p in parts]), y, M, row_scale, link, what, figures)


def from_z(z, bz, sigma, y, M=None, row_scale=None, link=0, what="", figures=None):
    z = np.asarray(z, dtype=np.float64)
    rows, S = z.shape
    sd = None
    if not link:
        rs = np.ones(rows) if row_scale is None else np.asarray(row_scale, dtype=np.float64)
        sd = rs[:, None] * np.asarray(sigma, dtype=np.float64)[None, :]          # fl(sigma * row_scale) in double, as the device forms it
    sref, sbound = pp.score(z, bz, y, sd, link, figures)
    ref, bound, compared = from_l(sref["l"], sbound["l"], tail_len(S) if M is None else M, what, figures=figures)
    ref["l"] = sref["l"]
    return ref, bound, compared


def assert_loo(got, ref, bound, compared, what, report=print):
    """A Sampler.predict_loo result against from_l(): every compared row of every output within BOUND_FACTOR x its bound (the +inf of pareto_k must
    match exactly); the rows left out still finite (pareto_k: finite or +inf).  The ratios are printed before they are asserted."""
    ratios = {}
    for key in OUTPUTS:
        v = got[key]
        assert v is not None and v.shape == ref[key].shape, (what, key)
        if key == "pareto_k":
            assert not np.any(np.isnan(v)) and not np.any(v == -np.inf), (what, "pareto_k is neither finite nor +inf")
            inf = np.isinf(ref[key])
            assert np.array_equal(np.isinf(v)[compared], inf[compared]), f"{what}: the branch (smoothed against +inf) differs on a compared row"
            sel = compared & ~inf
        else:
            assert np.all(np.isfinite(v)), (what, key, "not finite")
            sel = compared
        ratios[key] = bound_ratio(v[sel], ref[key][sel], bound[key][sel])
    info = got["info"]
    report(f"predict_loo {what}: route {info['route']}, {info['chunks']} chunk(s) of {info['rows_per_chunk']} rows, {info['rows_per_sort']} row(s) per "
           f"workgroup at {info['padded_draws']} padded draws, tail {got['tail_len']}, {int((~compared).sum())} row(s) left out, "
           f"khat {np.min(got['pareto_k']):.3g} .. {np.max(np.where(np.isinf(got['pareto_k']), -np.inf, got['pareto_k'])):.3g}, "
           "max |device - model| / bound: " + ", ".join(f"{k} {r:.3g}" for k, r in ratios.items()))
    for key, r in ratios.items():
        assert r <= BOUND_FACTOR, f"{what}: {key} is {r:.3g} x the bound (allowed: {BOUND_FACTOR:g})"
    return ratios


def device_bytes_formula(P, rows, nodes, S, T, offset, M, E, q, C, link, row_scale, outputs):
    """the device memory of one call (every allocation at least 16 bytes).  The only rows-times-draws term is the chunk's: 8 C S."""
    sizes = [2 * P * rows, 24 * nodes, 8 * S * T, 16 * S, 8 * C * S, 8 * rows]          # binned rows, nodes, tree starts, scales, values, y
    if offset:
        sizes.append(8 * rows)
    if M:
        sizes += [8 * rows * M, 8 * S * M]
    if E:
        sizes += [4 * rows * E, 8 * rows * E, 8 * S * q]
    if not link:
        sizes += [8 * S] + ([8 * rows] if row_scale else [])
    sizes += [8 * rows] * outputs
    return sum(max(16, t) for t in sizes)


def lds_bytes(S, M):
    """the dynamic LDS of a k_loo_rows launch."""
    sp = 1 << max(0, int(S) - 1).bit_length()
    R = max(1, 4096 // sp)
    slots = 4 if R >= 4 else R
    return 8 * max(sp, 4096) + 8 * 32 + 8 * slots * M


def synthetic(S, rows, seed, heavy=0.25):
    """A normal-likelihood case without a chain: z [rows x S] around a row level, sigma [S], y a few sd out for a share `heavy` of the rows (the
    heavy-tail regime: khat beyond 0.7) and within one sd for the others."""
    g = np.random.default_rng([31337, S, rows, seed])
    z = g.normal(size=(rows, 1)) + 0.3 * g.standard_normal((rows, S))
    sigma = g.uniform(0.4, 0.8, S)
    far = g.uniform(size=rows) < heavy
    y = z.mean(axis=1) + np.where(far, g.uniform(1.5, 4.0, rows) * g.choice([-1.0, 1.0], rows), g.normal(size=rows) * 0.5)
    return z, sigma, y
