#!/usr/bin/env python3
"""What the posterior predictive read-out of a finished fit costs on the GPU box: s4b_predict_ppd (dev_ppd.inc: k_predict_values unchanged, then per
chunk k_ppd_rows — the row reductions of the scores, Philox and Box-Muller in registers, the LDS sort) against
    (a) s4b_predict_quantiles of the same shape on the same build: what the added work — the noise and four row reductions — costs beside the sort;
    (b) the host way: predict_bart in row chunks, numpy's own normal deviates times sigma (no Philox on the host: a user would not write one),
        np.quantile along the draws, and for the scores a numpy log-sum-exp and the two moments (no PIT: numpy has no normal cdf).
One stationary chain of the benchmark's Friedman shape supplies the kept trees (tools/contrast_probe.py's chain).
    python tools/ppd_probe.py [--rows 100000] [--draws 100] [--pool 1 4] [--out profiles/predict_ppd.txt]
Per pool size: the call with quantiles only, the call with quantiles and scores, (a) and (b) (while its matrix stays below --host-gb).  One warm-up
call of each variant, then the variants alternating with --gap seconds of rest in front of every timed call (tools/contrast_probe.py says why),
medians and min-max.  Wall clock around the calls, which end in a stream synchronise: binning of the rows on the host, uploads, kernels and
downloads are inside for every variant.  The scores of (b) are compared with the device's before the times are reported; its quantiles belong to
another draw of the noise and are compared in distribution only (the mean width of the central 95 % interval)."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PROBS = (0.025, 0.5, 0.975)
Q_ONLY, Q_SCORES, QUANT, HOST = "ppd: quantiles", "ppd: quantiles and scores", "(a) predict_quantiles", "(b) predict_bart + numpy"


def new_rows(xb, m, seed):
    g = np.random.default_rng(seed)
    lo, hi = xb.min(axis=0), xb.max(axis=0)
    out = np.empty((m, xb.shape[1]), order="F")
    for j in range(xb.shape[1]):
        out[:, j] = g.uniform(lo[j], hi[j], m)
    return out


def host_way(s, x, y, sigma, times, chunk_rows, g):
    """predict_bart per chunk of rows (one [chunk x draws] matrix through the host), the same sampler's draws once per member of the pool, numpy's
    normal deviates, np.quantile; log-sum-exp and moments of the pointwise log-likelihood."""
    n, S = len(x), len(sigma)
    q, lpd, lmean, lm2 = np.empty((len(PROBS), n)), np.empty(n), np.empty(n), np.empty(n)
    for r0 in range(0, n, chunk_rows):
        z = np.tile(s.predict_bart(np.asfortranarray(x[r0:r0 + chunk_rows])), (1, times))
        sl = slice(r0, r0 + len(z))
        q[:, sl] = np.quantile(z + sigma[None, :] * g.standard_normal(z.shape), PROBS, axis=1)
        r = (y[sl, None] - z) / sigma[None, :]
        l = -0.5 * math.log(2.0 * math.pi) - np.log(sigma)[None, :] - 0.5 * r * r
        m = l.max(axis=1)
        lpd[sl] = m + np.log(np.exp(l - m[:, None]).sum(axis=1)) - math.log(S)
        lmean[sl] = l.mean(axis=1)
        lm2[sl] = ((l - lmean[sl, None]) ** 2).sum(axis=1)
    return dict(quantiles=q, lpd=lpd, lmean=lmean, lm2=lm2)


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
            pool = dict(peers=[s] * (times - 1))
            ppd = dict(sigma=sig[0], peer_sigma=sig[1:], noise_key=12345, **pool)
            variants = {Q_ONLY: lambda: s.predict_ppd(xn, PROBS, **ppd), Q_SCORES: lambda: s.predict_ppd(xn, PROBS, y=y, **ppd),
                        QUANT: lambda: s.predict_quantiles(xn, PROBS, **pool)}
            host = 8.0 * a.rows * S <= a.host_gb * 2 ** 30
            if host:
                variants[HOST] = lambda: host_way(s, xn, y, np.concatenate(sig), times, max(1000, (1 << 27) // (8 * S)), np.random.default_rng(3))
            res = {k: f() for k, f in variants.items()}                    # warm-up: code objects, allocator, page faults of the outputs
            i = res[Q_SCORES]["info"]
            say(f"rows={a.rows}, pooled draws={S} ({times} x {a.draws}): route {i['route']}, {i['chunks']} chunk(s) of {i['rows_per_chunk']} rows, "
                f"{i['rows_per_sort']} row(s) per workgroup of k_ppd_rows at {i['padded_draws']} padded draws, {i['launches']} launches, device memory "
                f"{i['device_bytes'] / 1e6:.1f} MB; the [rows x draws] matrix would be {8e-6 * a.rows * S:.0f} MB")
            assert np.array_equal(res[Q_ONLY]["quantiles"], res[Q_SCORES]["quantiles"])
            if host:
                h, dv = res[HOST], res[Q_SCORES]
                say("    (b) vs the device: max abs diff " + ", ".join(f"{k} {np.max(np.abs(h[k] - dv[k])):.2e}" for k in ("lpd", "lmean", "lm2"))
                    + f"; mean width of the central 95 % interval {np.mean(h['quantiles'][2] - h['quantiles'][0]):.4f} (b), "
                    f"{np.mean(dv['quantiles'][2] - dv['quantiles'][0]):.4f} (device: another draw of the noise)")
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
            say(f"    quantiles only / (a) = {med[Q_ONLY] / med[QUANT]:.2f}, with scores / (a) = {med[Q_SCORES] / med[QUANT]:.2f}"
                + (f", (b) / with scores = {med[HOST] / med[Q_SCORES]:.2f}, (b) / quantiles only = {med[HOST] / med[Q_ONLY]:.2f}" if host else ""))
            write()
    finally:
        s.free()
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
