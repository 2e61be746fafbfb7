"""s4b_predict_convergence (stan4bart_amd/csrc/dev_conv.inc: k_predict_values<staged / global> unchanged, k_chain_rows) — the model, the
bound, the rule for rows left out and the cases shared by tests/test_predict_convergence.py (CPU) and tests/test_gpu_predict_convergence.py (GPU).

THE MODEL (`estimate`) is numpy in long double on the FULL [rows x pooled draws] matrix and applies the definition of include/stan4bart_amd.h
literally: the chains gathered by their starts, the chain means (a chain whose minimum equals its maximum has that value as its mean, the device's exact
rule for a constant chain), W, var+, rhat, the autocovariances formed DIRECTLY lag by lag with divisor N, the pair rule, tau, ess, mean, mcse.  Lags are
formed only while some row still needs them.

THE BOUND of an entry has two parts; the tests allow readout_cases.BOUND_FACTOR x their sum.
  measured  the map x -> (J, tau) has no closed Lipschitz constant (a minimum, a truncation).  For it the MODEL'S OWN SENSITIVITY is taken: the
            long-double model is evaluated on x + s bx under PATTERNS seeded sign patterns s (bx: what the device's value kernel — and for quantity 1
            its log-likelihood and exponential — may add to an element), each run also moving every intermediate by the arithmetic error of the
            kernel's stated summation order (u = 2^-53; Ll = ceil(N / 64) + 6 the additions of a lane-strided sum with the butterfly over a chain,
            Lc = ceil(C / 64) + 6 the same over the chains):
              mu_c     (Ll + 1) u mean|x|                          q_c      relative (Ll + 4) u  (d rounds, its square, the sum)
              sum q    relative Lc u                                mean     (Lc + 1) u mean|mu_c|
              sum (mu_c - mean)^2  relative (Lc + 4) u              W        relative 2 u          var+   relative 4 u
              G(t)     (ceil((N - t) / 4) + 6 + ceil(C / 4) + 2) u sum_c sum_i |d_c[i] d_c[i+t]|  (two rounded factors, the product, four partial
                       sums, their fold, the chains in four groups, their fold)
              rho(t)   u ((|m| + 2 |W - m|) / var+ + |rho|), m = G / D  (the quotient, the difference, the quotient, the difference)
            and once more in float64 without jitter.  The largest deviation from the long-double model over these runs is the measured part.  Measured
            against the reference, never against the device.
  derived   the last operations, J the model's: tau carries (J // 32 + 9) additions of the P'_j and three more operations,
              ess   relative u (2 (J // 32 + 9) (sum |P'_j| + |e'_J|) + 3 |tau| + 2) / |tau| + (2 k_log + 3) u
              rhat  relative 3 u          mean  u |mean|          mcse  relative half of ess's + (Lc + 8) u
A row is LEFT OUT of the numeric comparison where these runs disagree on J (this covers a pair J whose sum changes sign and a running minimum that
changes hands only in so far as they move the values, which the measured part then holds) or on whether the row has an answer; `from_x` asserts that
at most 2 % of a case's rows are.  For every compared row n_pairs must equal the model's J exactly.  A row WITHOUT an answer in the model (N < 4, a
value that is not finite, every chain exactly constant) must be NaN / -1 on the device."""
import math

import numpy as np

import latent_par_cases as lp
import ppd_cases as pp
from readout_cases import BOUND_FACTOR, U, bound_ratio  # noqa: F401

LD = np.longdouble
OUTPUTS = ("rhat", "ess", "mean", "mcse")
CHAINS_MAX = 256
DRAWS_MAX = 16384
LAGS = 64                   # lags of a block of k_chain_rows: 32 pairs
PATTERNS = 8
LEFT_OUT_MAX = 0.02


def chains(lens, split=True):
    """(starts, N) of the chains of pooled samplers with `lens` kept draws: each cut to the shortest, with `split` halved (the middle draw of an odd
    length dropped) — SamplerCore::conv_chains."""
    n0 = min(int(n) for n in lens)
    h = n0 // 2
    starts, at = [], 0
    for n in lens:
        starts.append(at)
        if split:
            starts.append(at + n0 - h)
        at += int(n)
    return starts, (h if split else n0)


def j_limit(N):
    """The first j with 2 j + 1 >= N - 4: the pair the sequence stops at whatever the data."""
    return max(0, (int(N) - 4) // 2)


def lag_products(d, t):
    """d [rows x C x N] -> d[i] d[i + t] over i < N - t: [rows x C x (N - t)]."""
    N = d.shape[2]
    return d[:, :, :N - t] * d[:, :, t:]


def acov(d, t):
    """a_c(t) = sum_{i < N - t} d[i] d[i + t] / N of the centred chains d [rows x C x N]: divisor N at every lag."""
    return lag_products(d, t).sum(axis=2) / d.dtype.type(d.shape[2])


def estimate(x, starts, N, dtype=LD, jitter=None):
    """The definition applied to x [rows x S] with chains of N draws beginning at `starts`, in `dtype`.  `jitter`: None or a Generator whose signs
    move the intermediates by their arithmetic error (module docstring).  Returns dict(rhat, ess, mean, mcse, tau [rows] in dtype, n_pairs [rows]
    int (-1: no answer), answer [rows] bool, abs_terms: sum_{j<J} |P'_j| + |e'_J|)."""
    x = np.asarray(x).astype(dtype)
    rows, C = x.shape[0], len(starts)
    D = C * N
    nan = np.full(rows, np.nan, dtype=dtype)
    out = dict(rhat=nan.copy(), ess=nan.copy(), mean=nan.copy(), mcse=nan.copy(), tau=nan.copy(), n_pairs=np.full(rows, -1, dtype=np.int64),
               answer=np.zeros(rows, dtype=bool), abs_terms=np.zeros(rows))
    if N < 4:
        return out
    sign = (lambda shape: jitter.choice([-1.0, 1.0], size=shape).astype(dtype) * dtype(U)) if jitter is not None else None
    Ll, Lc = -(-N // 64) + 6, -(-C // 64) + 6
    X = x[:, np.asarray(starts)[:, None] + np.arange(N)[None, :]]          # [rows x C x N]
    finite = np.isfinite(X).all(axis=(1, 2))
    X = np.where(finite[:, None, None], X, dtype(0))
    with np.errstate(all="ignore"):
        const = X.min(axis=2) == X.max(axis=2)
        mu = np.where(const, X[:, :, 0], X.sum(axis=2) / dtype(N))
        if sign is not None:
            mu = mu + np.where(const, dtype(0), sign(mu.shape) * (Ll + 1) * np.abs(X).mean(axis=2))
        d = X - mu[:, :, None]
        q = (d * d).sum(axis=2)
        if sign is not None:
            q = q * (1 + sign(q.shape) * (Ll + 4))
        sq, mean = q.sum(axis=1), mu.sum(axis=1) / dtype(C)
        if sign is not None:
            sq = sq * (1 + sign(rows) * Lc)
            mean = mean + sign(rows) * (Lc + 1) * np.abs(mu).mean(axis=1)
        e = mu - mean[:, None]
        sb = (e * e).sum(axis=1)
        if sign is not None:
            sb = sb * (1 + sign(rows) * (Lc + 4))
        W = sq / dtype((N - 1) * C)
        vp = W * dtype(N - 1) / dtype(N) + (sb / dtype(C - 1) if C > 1 else dtype(0))
        if sign is not None:
            W, vp = W * (1 + sign(rows) * 2), vp * (1 + sign(rows) * 4)
        ok = finite & (W > 0) & np.isfinite(vp)

        def rho(t, ra):
            if t == 0:
                return np.ones(len(ra), dtype=dtype)
            p = lag_products(d[ra], t)
            G = p.sum(axis=(1, 2))
            if sign is not None:
                G = G + sign(len(ra)) * (-(-(N - t) // 4) + 6 + -(-C // 4) + 2) * np.abs(p).sum(axis=(1, 2))
            m = G / dtype(D)
            r = 1 - (W[ra] - m) / vp[ra]
            if sign is not None:
                r = r + sign(len(ra)) * ((np.abs(m) + 2 * np.abs(W[ra] - m)) / vp[ra] + np.abs(r))
            return r

        jm = j_limit(N)
        active = ok.copy()
        J = np.full(rows, -1, dtype=np.int64)
        sumP, absP = np.zeros(rows, dtype=dtype), np.zeros(rows, dtype=dtype)
        pmin = np.full(rows, np.inf, dtype=dtype)
        eJ, PJ = np.ones(rows, dtype=dtype), np.zeros(rows, dtype=dtype)
        for j in range(jm + 1):
            ra = np.nonzero(active)[0]
            if not len(ra):
                break
            ev, od = rho(2 * j, ra), rho(2 * j + 1, ra)
            P = ev + od
            stop = ~(P > 0) | (j >= jm)
            st, go = ra[stop], ra[~stop]
            J[st], eJ[st], PJ[st] = j, ev[stop], P[stop]
            pm = np.minimum(pmin[go], P[~stop])
            pmin[go] = pm
            sumP[go] += pm
            absP[go] += np.abs(pm)
            active[st] = False
        assert not active.any()
        eSt = np.where(J == 0, dtype(1), np.where(PJ >= 0, eJ, dtype(0)))
        tau = -1 + 2 * (sumP + eSt) + np.where(eJ > 0, eJ, dtype(0))
        ess = np.minimum(dtype(D) / tau, dtype(D) * np.log10(dtype(D)))
        mcse = np.sqrt((sq + dtype(N) * sb) / dtype(D - 1)) / np.sqrt(ess)
        rhat = np.sqrt(vp / W) if C > 1 else nan
    for key, v in (("rhat", rhat), ("ess", ess), ("mean", mean), ("mcse", mcse), ("tau", tau)):
        out[key] = np.where(ok, v, dtype(np.nan))
    out["n_pairs"] = np.where(ok, J, -1)
    out["answer"] = ok
    out["abs_terms"] = (absP + np.abs(eSt)).astype(np.float64)
    return out


def from_x(x, bx, starts, N, what="", left_out_max=LEFT_OUT_MAX, figures=None):
    """(ref, bound, compared) of the series x [rows x S] known to within bx: ref holds OUTPUTS as float64 [rows], n_pairs and answer; `compared` [rows]
    is False where the model has no answer or the perturbed models disagree on J.  Asserts that at most left_out_max of the rows WITH an answer are
    left out."""
    k = lp.DEVICE if figures is None else figures
    x = np.asarray(x, dtype=np.float64)
    bx = np.broadcast_to(np.asarray(bx, dtype=np.float64), x.shape)
    rows, C = x.shape[0], len(starts)
    base = estimate(x, starts, N)
    runs = [estimate(x, starts, N, dtype=np.float64)]
    g = np.random.default_rng([20250, C, N, rows])
    for _ in range(PATTERNS):
        s = g.choice([-1.0, 1.0], size=x.shape)
        runs.append(estimate(x.astype(LD) + (s * bx).astype(LD), starts, N, jitter=g))
    compared = base["answer"].copy()
    dev = {key: np.zeros(rows) for key in OUTPUTS}
    for r in runs:
        compared &= (r["n_pairs"] == base["n_pairs"]) & r["answer"]
        with np.errstate(all="ignore"):
            for key in OUTPUTS:
                dd = np.abs(np.asarray(r[key], dtype=LD) - base[key]).astype(np.float64)
                dev[key] = np.maximum(dev[key], np.where(np.isfinite(dd), dd, 0.0))
    left = int((base["answer"] & ~compared).sum())
    assert left <= left_out_max * rows, f"{what}: {left} of {rows} rows change J under the perturbed models (allowed: 2 %)"
    f = {key: np.asarray(base[key], dtype=np.float64) for key in OUTPUTS}
    Lc = -(-C // 64) + 6
    with np.errstate(all="ignore"):
        J = np.maximum(base["n_pairs"], 0)
        tau = np.abs(np.asarray(base["tau"], dtype=np.float64))
        rel_ess = U * (2.0 * (J // 32 + 9) * base["abs_terms"] + 3.0 * tau + 2.0) / tau + (2.0 * k["log"] + 3.0) * U
        arith = dict(rhat=3.0 * U * np.abs(f["rhat"]), ess=np.abs(f["ess"]) * rel_ess, mean=U * np.abs(f["mean"]),
                     mcse=np.abs(f["mcse"]) * (0.5 * rel_ess + (Lc + 8.0) * U))
    bound = {key: dev[key] + np.where(np.isfinite(arith[key]), arith[key], 0.0) for key in OUTPUTS}
    ref = dict(f, n_pairs=base["n_pairs"], answer=base["answer"])
    return ref, bound, compared


def lik_series(l, bl, figures=None):
    """Quantity 1: (x, bx) = exp(l - max_k l) of the log-likelihoods l [rows x S] known to within bl, the maximum over ALL pooled draws, rounded to
    double as the device holds it (below exp(-745) it is 0 there).  An element moves by its own l, by the maximum's, by the rounded difference and by
    the exponential."""
    k = lp.DEVICE if figures is None else figures
    l = np.asarray(l, dtype=np.float64)
    bl = np.broadcast_to(np.asarray(bl, dtype=np.float64), l.shape)
    with np.errstate(all="ignore"):
        am = np.nanargmax(np.where(np.isnan(l).all(axis=1, keepdims=True), 0.0, l), axis=1)
        mx = l[np.arange(len(l)), am][:, None]
        dl = l.astype(LD) - mx.astype(LD)
        x = np.exp(dl).astype(np.float64)
        bx = x * (bl + bl[np.arange(len(l)), am][:, None] + U * np.abs(dl).astype(np.float64) + 2.0 * k["exp"] * U)
    return x, np.where(np.isfinite(bx), bx, 0.0)


def model(parts, starts, N, quantity=0, y=None, row_scale=None, link=0, offset=None, dense=None, ell_index=None, ell_value=None, what="", figures=None):
    """`parts` as ppd_cases.model takes them (quantity 1, link 0: each with its sigma).  from_x of the pooled series."""
    import summary_cases as sc
    if quantity == 0:
        vs, bs = [], []
        for p in parts:
            ref, bd = sc.model(p["bart"], offset, dense, p.get("dense_coef"), ell_index, ell_value, p.get("ell_coef"), link=link)
            vs.append(ref["v"])
            bs.append(np.broadcast_to(bd["v"], ref["v"].shape))
        x, bx = np.concatenate(vs, axis=1), np.concatenate(bs, axis=1)
    else:
        z, bz = pp.pooled_z(parts, offset, dense, ell_index, ell_value)
        sd = None
        if not link:
            rs = np.ones(len(z)) if row_scale is None else np.asarray(row_scale, dtype=np.float64)
            sd = rs[:, None] * np.concatenate([np.asarray(p["sigma"], dtype=np.float64) for p in parts])[None, :]
        sref, sbound = pp.score(z, bz, y, sd, link, figures)
        x, bx = lik_series(sref["l"], sbound["l"], figures)
    ref, bound, compared = from_x(x, bx, starts, N, what, figures=figures)
    ref["x"] = x
    return ref, bound, compared


def assert_conv(got, ref, bound, compared, what, report=print):
    """A Sampler.predict_convergence result against from_x(): every compared row of every output within BOUND_FACTOR x its bound and n_pairs equal to
    the model's J; a row without an answer in the model NaN / -1; a row left out still with an answer.  The ratios are printed before they are
    asserted."""
    ratios = {}
    none = ~ref["answer"]
    C = got["chains"]
    for key in OUTPUTS:
        v = got[key]
        assert v is not None and v.shape == ref[key].shape, (what, key)
        assert np.all(np.isnan(v[none])), f"{what}: {key} of a row without an answer is not NaN"
        if key == "rhat" and C == 1:
            assert np.all(np.isnan(v)), f"{what}: rhat of one chain is not NaN"
            continue
        sel = compared
        if key == "mcse":          # the root of a negative ess (a negative tau: short antithetic chains) is NaN on both sides
            neg = ~none & (got["ess"] < 0)
            assert np.array_equal(np.isnan(v[~none]), neg[~none]), f"{what}: mcse is NaN elsewhere than beside a negative ess"
            sel = compared & ~neg & np.isfinite(ref[key])
        else:
            assert not np.any(np.isnan(v[~none])), f"{what}: {key} is NaN in a row that has an answer"
        ratios[key] = bound_ratio(v[sel], ref[key][sel], bound[key][sel]) if sel.any() else 0.0
    if got["n_pairs"] is not None:
        assert np.array_equal(got["n_pairs"][none], np.full(int(none.sum()), -1)), f"{what}: n_pairs of a row without an answer is not -1"
        assert np.array_equal(got["n_pairs"][compared], ref["n_pairs"][compared]), f"{what}: n_pairs differs from the model's J on a compared row"
        assert np.all(got["n_pairs"][~none] >= 0) and np.all(got["n_pairs"][~none] <= j_limit(got["chain_len"]))
    info = got["info"]
    npairs = got["n_pairs"][~none] if got["n_pairs"] is not None and (~none).any() else np.zeros(1, dtype=int)
    report(f"predict_convergence {what}: route {info['route']}, {info['chunks']} chunk(s) of {info['rows_per_chunk']} rows, {info['rows_per_sort']} row(s) "
           f"per workgroup at {info['padded_draws']} padded draws, {got['chains']} chains of {got['chain_len']}, n_pairs {npairs.min()} .. {npairs.max()}, "
           f"{int((ref['answer'] & ~compared).sum())} row(s) left out, {int(none.sum())} without an answer, "
           "max |device - model| / bound: " + ", ".join(f"{k} {r:.3g}" for k, r in ratios.items()))
    for key, r in ratios.items():
        assert r <= BOUND_FACTOR, f"{what}: {key} is {r:.3g} x the bound (allowed: {BOUND_FACTOR:g})"
    return ratios


def device_bytes_formula(P, rows, nodes, S, T, offset, M, E, q, C, chains_, quantity, link, row_scale, outputs, n_pairs):
    """the device memory of one call (every allocation at least 16 bytes).  The only rows-times-draws term is the chunk's: 8 C S."""
    sizes = [2 * P * rows, 24 * nodes, 8 * S * T, 16 * S, 8 * C * S, 4 * chains_]          # binned rows, nodes, tree starts, scales, values, chain starts
    if offset:
        sizes.append(8 * rows)
    if M:
        sizes += [8 * rows * M, 8 * S * M]
    if E:
        sizes += [4 * rows * E, 8 * rows * E, 8 * S * q]
    if quantity:
        sizes += [8 * rows] + ([] if link else [8 * S] + ([8 * rows] if row_scale else []))
    sizes += [8 * rows] * outputs + ([4 * rows] if n_pairs else [])
    return sum(max(16, t) for t in sizes)


def lds_bytes(S, C):
    """the dynamic LDS of a k_chain_rows launch."""
    sp = 1 << max(0, int(S) - 1).bit_length()
    R = max(1, 4096 // sp)
    slots = 4 if R >= 4 else R
    return 8 * max(sp, 4096) + 8 * 16 + 16 * slots * C + 8 * slots * 4 * LAGS


# ---- series ---------------------------------------------------------------------------------------------------------------------------------------------
def ar1(phi, n, g, shape=()):
    """Stationary AR(1) series of unit innovation variance: [*shape x n]."""
    out = np.empty(tuple(shape) + (n,))
    out[..., 0] = g.standard_normal(shape) / math.sqrt(1.0 - phi * phi)
    for t in range(1, n):
        out[..., t] = phi * out[..., t - 1] + g.standard_normal(shape)
    return out


def synthetic(lens, rows, seed):
    """A case without a chain, of the shape of the GPU tests' ordinary rows: per row a level, per pooled sampler a small shift and an AR(1) series whose
    phi is drawn per row from (-0.5, 0.9).  Returns x [rows x sum(lens)]."""
    g = np.random.default_rng([4242, len(lens), min(lens), rows, seed])
    phi = g.uniform(-0.5, 0.9, rows)
    cols = []
    for n in lens:
        s = np.empty((rows, n))
        s[:, 0] = g.standard_normal(rows) / np.sqrt(1.0 - phi * phi)
        for t in range(1, n):
            s[:, t] = phi * s[:, t - 1] + g.standard_normal(rows)
        cols.append(s + 0.2 * g.standard_normal((rows, 1)))
    return g.normal(size=(rows, 1)) + 0.3 * np.concatenate(cols, axis=1)


# the pools of tests/test_gpu_predict_convergence.py: name -> (kept draws of the pooled samplers, split).  Lengths 3 .. 13 come from the short chain, 66 ..
# 2048 from the long one.  tests/test_predict_convergence.py shows the share left out at every one of them with the model alone.
POOLS = {
    "3": ((3, 3), False), "4": ((4, 4), False), "5": ((5, 5, 5), False), "6": ((6, 6), False), "7": ((7, 7), False), "8": ((8, 8), False),
    "9": ((9, 9), False), "13+5": ((13, 5), False), "6s": ((6, 6), True), "8s": ((8, 8), True), "9s": ((9, 9), True), "13s": ((13, 13), True),
    "13+9s": ((13, 9, 13), True), "1x13": ((13,), False), "1x13s": ((13,), True), "4x13s": ((13,) * 4, True), "128x9s": ((9,) * 128, True),
    "2x66": ((66, 66), False), "2x68": ((68, 68), False), "2x130": ((130, 130), False), "2x132": ((132, 132), False), "2x132s": ((132, 132), True),
    "7x132": ((132,) * 7, True), "9x132": ((132,) * 9, True), "17x132": ((132,) * 17, True), "8x2048": ((2048,) * 8, True),
}
