#!/usr/bin/env python3
"""What PSIS-LOO of a finished fit costs on the GPU box: s4b_predict_loo (dev_loo.inc: k_predict_values unchanged, then per chunk k_loo_rows — the
log-likelihood once per element, the LDS sort, the generalised-Pareto fit of the tail with one grid point per lane, four row sums) against
    (a) s4b_predict_ppd of the same shape on the same build with the scores (lpd, lmean, lm2, pit) and no probs: the two row kernels side by side
        behind the same value kernel — what the sort and the fit cost beside plain row reductions;
    (b) the host way: predict_bart in row chunks and a vectorised numpy PSIS in double (sort, the tail, the fit over the whole grid at once as a
        [rows x grid x tail] array in row blocks, the smoothed tail, the four outputs) — what a user of loo::loo() on the log-likelihood matrix pays.
One stationary chain of the benchmark's Friedman shape supplies the kept trees (tools/ppd_probe.py's chain).
    python tools/loo_probe.py [--rows 100000] [--draws 100] [--pool 1 4] [--out profiles/predict_loo.txt]
Per pool size: the call, (a) and (b) (while its matrix stays below --host-gb).  One warm-up call of each variant, then the variants alternating with
--gap seconds of rest in front of every timed call (tools/contrast_probe.py says why), medians and min-max.  Wall clock around the calls, which end
in a stream synchronise: binning of the rows on the host, uploads, kernels and downloads are inside for every variant.  The results of (b) are compared
with the device's before the times are reported."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LOO, PPD, HOST = "predict_loo", "(a) predict_ppd: scores", "(b) predict_bart + numpy PSIS"


def tail_len(S):
    m = math.isqrt(9 * S)
    return min(-(-S // 5), m + (m * m < 9 * S))


def psis_numpy(l, M, block_bytes=1 << 27):
    """The definition of include/stan4bart_amd.h (s4b_predict_loo) in double, vectorised over the rows of l [rows x S]."""
    rows, S = l.shape
    lr = np.sort(-l, axis=1)
    lw = lr - lr[:, -1:]
    khat = np.full(rows, np.inf)
    if M >= 5:
        G = 30 + math.isqrt(M)
        g = np.arange(1, G + 1)
        p = (np.arange(M) + 0.5) / M
        step = max(1, block_bytes // (8 * G * M))
        with np.errstate(all="ignore"):
            for r0 in range(0, rows, step):
                t = lw[r0:r0 + step, S - M:]
                ec = np.exp(lw[r0:r0 + step, S - M - 1])[:, None]
                x = np.exp(t) - ec
                theta = 1.0 / x[:, -1:] + (1.0 - np.sqrt(G / (g - 0.5)))[None, :] / (3.0 * x[:, int(math.floor(M / 4.0 + 0.5)) - 1][:, None])
                kap = np.log1p(-theta[:, :, None] * x[:, None, :]).mean(axis=2)
                L = M * (np.log(-theta / kap) - kap - 1.0)
                e = np.exp(L - L.max(axis=1, keepdims=True))
                th = (theta * e).sum(axis=1) / e.sum(axis=1)
                k0 = np.log1p(-th[:, None] * x).mean(axis=1)
                sg, kh = -k0 / th, k0 * M / (M + 10.0) + 5.0 / (M + 10.0)
                ok = np.isfinite(kh) & np.isfinite(sg) & (t[:, -1] - t[:, 0] >= 2.0 ** -52 / 100.0)
                sm = np.minimum(0.0, np.log(sg[:, None] * np.expm1(-kh[:, None] * np.log1p(-p)[None, :]) / kh[:, None] + ec))
                lw[r0:r0 + step, S - M:] = np.where(ok[:, None], sm, t)
                khat[r0:r0 + step] = np.where(ok, kh, np.inf)

    def lse(a):
        m = a.max(axis=1)
        return m + np.log(np.exp(a - m[:, None]).sum(axis=1))
    w = np.exp(lw)
    return dict(elpd_loo=lse(lw - lr) - lse(lw), pareto_k=khat, lpd=lse(-lr) - math.log(S), ess=w.sum(axis=1) ** 2 / (w * w).sum(axis=1))


def host_way(s, x, y, sigma, times, chunk_rows):
    """predict_bart per chunk of rows (one [chunk x draws] matrix through the host), the same sampler's draws once per member of the pool, the normal
    log-likelihood, psis_numpy."""
    n, S = len(x), len(sigma)
    out = {k: np.empty(n) for k in ("elpd_loo", "pareto_k", "lpd", "ess")}
    for r0 in range(0, n, chunk_rows):
        z = np.tile(s.predict_bart(np.asfortranarray(x[r0:r0 + chunk_rows])), (1, times))
        r = (y[r0:r0 + len(z), None] - z) / sigma[None, :]
        l = -0.5 * math.log(2.0 * math.pi) - np.log(sigma)[None, :] - 0.5 * r * r
        for k, v in psis_numpy(l, tail_len(S)).items():
            out[k][r0:r0 + len(z)] = v
    return out


def fmt(ts):
    return f"median {statistics.median(ts) * 1e3:9.2f} ms  (min {min(ts) * 1e3:9.2f}, max {max(ts) * 1e3:9.2f}, {len(ts)} calls)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000, help="training rows of the chain")
    ap.add_argument("--p", type=int, default=51, help="columns of the Friedman design (one goes to the fixed part: p - 1 BART predictors)")
    ap.add_argument("--trees", type=int, default=200)
    ap.add_argument("--burn-in", type=int, default=1000)
    ap.add_argument("--draws", type=int, default=100)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--pool", type=int, nargs="+", default=[1, 4], help="times the sampler is pooled with itself")
    ap.add_argument("--host-gb", type=float, default=1.0, help="the host way is timed while 8 x rows x pooled draws stays below this")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gap", type=float, default=0.3, help="seconds of rest in front of every timed call, outside the timed window (0: back to back)")
    ap.add_argument("--limit", type=float, default=90.0, help="seconds one timed step may take before the probe gives up")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ppd_probe import new_rows
    from stan4bart_amd import GroupTerm, RRng, generate_friedman_data, make_sampler_args
    from stan4bart_amd._lib import load_library
    from stan4bart_amd.abi import Sampler
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def write():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    d = generate_friedman_data(a.n, ranef=True, causal=True, p=a.p)
    x = d["x"]
    xb = np.asfortranarray(x[:, [j for j in range(a.p) if j != 3]])
    args = make_sampler_args(d["y"], xb, X=np.column_stack([x[:, 3], d["z"]]), groups=[GroupTerm(d["g1"], x[:, 3], "g.1"), GroupTerm(d["g2"], None, "g.2")],
                             iter=a.burn_in + a.draws, warmup=a.burn_in, keep_fits=False, bart_args={"n.trees": a.trees, "keepTrees": True})
    rng = RRng(99)
    args.seed = int(rng.sample_int(2147483647, 1)[0])
    s = Sampler(load_library(), "s4b_", args, rng.state)
    try:
        t0 = time.perf_counter()
        s.run(a.burn_in, True, 0)
        s.disengage_adaptation()
        s.run(a.draws, False, 0)
        say(f"library {os.environ.get('S4B_LIB_PATH', 'libs4b.so')}; chain: Friedman n={a.n}, {xb.shape[1]} BART predictors, {a.trees} trees, "
            f"{a.burn_in} warm-up + {a.draws} kept draws in {time.perf_counter() - t0:.1f} s")
        xn = new_rows(xb, a.rows, 1)
        g = np.random.default_rng(2)
        y = s.predict_bart(np.asfortranarray(xn))[:, 0] + g.standard_normal(a.rows)
        for times in a.pool:
            S = a.draws * times
            sig = [g.uniform(0.8, 1.2, a.draws) for _ in range(times)]
            pool = dict(y=y, sigma=sig[0], peer_sigma=sig[1:], peers=[s] * (times - 1))
            variants = {LOO: lambda: s.predict_loo(xn, **pool), PPD: lambda: s.predict_ppd(xn, (), **pool)}
            host = 8.0 * a.rows * S <= a.host_gb * 2 ** 30
            if host:
                variants[HOST] = lambda: host_way(s, xn, y, np.concatenate(sig), times, max(1000, (1 << 27) // (8 * S)))
            res = {k: f() for k, f in variants.items()}                    # warm-up: code objects, allocator, page faults of the outputs
            i, dv = res[LOO]["info"], res[LOO]
            fin = np.isfinite(dv["pareto_k"])
            say(f"rows={a.rows}, pooled draws={S} ({times} x {a.draws}), tail {dv['tail_len']}: route {i['route']}, {i['chunks']} chunk(s) of {i['rows_per_chunk']} rows, "
                f"{i['rows_per_sort']} row(s) per workgroup of k_loo_rows at {i['padded_draws']} padded draws, {i['launches']} launches, device memory "
                f"{i['device_bytes'] / 1e6:.1f} MB; the [rows x draws] matrix would be {8e-6 * a.rows * S:.0f} MB")
            say(f"    elpd_loo total {dv['elpd_loo'].sum():.3f}, p_loo total {(dv['lpd'] - dv['elpd_loo']).sum():.3f}, khat {dv['pareto_k'][fin].min():.3f} .. "
                f"{dv['pareto_k'][fin].max():.3f} ({np.mean(dv['pareto_k'] > 0.7):.2%} of the rows above 0.7, {np.mean(~fin):.2%} without a fit); "
                f"lpd against (a): max abs diff {np.max(np.abs(dv['lpd'] - res[PPD]['lpd'])):.2e}")
            if host:
                h = res[HOST]
                same = np.isfinite(h["pareto_k"]) == fin
                with np.errstate(invalid="ignore"):
                    diff = {k: np.abs(h[k] - dv[k])[same & (fin | (k != "pareto_k"))] for k in ("elpd_loo", "pareto_k", "lpd", "ess")}          # (inf - inf where neither fitted)
                say(f"    (b) vs the device: the same branch in {same.mean():.4%} of the rows; there max abs diff " + ", ".join(f"{k} {v.max():.2e}" for k, v in diff.items()))
            ts = {k: [] for k in variants}
            for _ in range(a.reps):                                        # alternating: drifts of the shared host hit every variant alike
                for k, f in variants.items():
                    time.sleep(a.gap)
                    t0 = time.perf_counter()
                    f()
                    ts[k].append(time.perf_counter() - t0)
                    if ts[k][-1] > a.limit:
                        say(f"    {k}: a call took {ts[k][-1]:.1f} s, beyond the limit of {a.limit:.0f} s: giving up")
                        write()
                        return 1
            for k in variants:
                say(f"    {k:40s} {fmt(ts[k])}")
            med = {k: statistics.median(v) for k, v in ts.items()}
            say(f"    predict_loo / (a) = {med[LOO] / med[PPD]:.2f}" + (f", (b) / predict_loo = {med[HOST] / med[LOO]:.2f}" if host else ""))
            write()
    finally:
        s.free()
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
