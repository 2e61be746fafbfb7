#!/usr/bin/env python3
"""What split R-hat and the effective sample size of every row cost on the GPU box: s4b_predict_convergence (dev_conv.inc: k_predict_values unchanged,
then per chunk k_chain_rows — the rows in LDS as plain doubles, the chain sums, the autocovariances formed directly in blocks of 64 lags, one lag per
lane, until Geyer's sequence stops) against
    (a) s4b_predict_quantiles of the same shape on the same build (three probs): the two row kernels side by side behind the same value kernel — what
        the chain kernel costs beside the LDS sort;
    (b) the host way: predict_bart in row chunks and a vectorised numpy version of the same estimator (one FFT per row and chain for the
        autocovariances at every lag, the pair rule over all rows at once) — what a user pays who runs Stan's estimator on the draws matrix.
One stationary chain of the benchmark's Friedman shape supplies the kept trees (tools/ppd_probe.py's chain); it is pooled with itself, every occurrence
with a per-draw series of its own added through one dense column, so that the chains differ.  --sticky PHI makes that series an AR(1) of coefficient
PHI that dominates the trees: every row then needs many blocks of lags.
    python tools/convergence_probe.py [--rows 100000] [--draws 25 100] [--pool 4] [--sticky 0.99] [--out profiles/predict_convergence.txt]
Per shape: the call, (a) and (b) (while its matrix stays below --host-gb).  One warm-up call of each variant, then the variants alternating with --gap
seconds of rest in front of every timed call (tools/contrast_probe.py says why), medians and min-max.  Wall clock around the calls, which end in a
stream synchronise: binning of the rows on the host, uploads, kernels and downloads are inside for every variant.  The results of (b) are compared
with the device's before the times are reported.  Kernel times: run the probe under a kernel trace with --reps 1 (profiles/predict_convergence.txt)."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CONV, QUANT, HOST = "predict_convergence", "(a) predict_quantiles", "(b) predict_bart + numpy FFT"


def estimator_numpy(x, C, N):
    """The definition of include/stan4bart_amd.h (s4b_predict_convergence) in double for x [rows x C x N], the autocovariances by FFT."""
    rows = len(x)
    D = C * N
    mu = x.mean(axis=2)
    d = x - mu[:, :, None]
    f = np.fft.rfft(d, 2 * N, axis=2)
    A = np.fft.irfft(f.real ** 2 + f.imag ** 2, 2 * N, axis=2)[:, :, :N]          # lag sums, every lag
    W = A[:, :, 0].sum(axis=1) / ((N - 1) * C)
    mean = mu.mean(axis=1)
    sb = ((mu - mean[:, None]) ** 2).sum(axis=1)
    vp = W * (N - 1) / N + (sb / (C - 1) if C > 1 else 0.0)
    with np.errstate(all="ignore"):
        rho = 1.0 - (W[:, None] - A.sum(axis=1) / D) / vp[:, None]
        rho[:, 0] = 1.0
        jm = max(0, (N - 4) // 2)
        ev, od = rho[:, 0:2 * jm + 2:2], rho[:, 1:2 * jm + 2:2]
        P = ev + od
        stop = ~(P > 0)
        stop[:, jm] = True
        J = stop.argmax(axis=1)
        run = np.minimum.accumulate(np.where(np.isnan(P), np.inf, P), axis=1)
        sumP = np.where(np.arange(jm + 1)[None, :] < J[:, None], run, 0.0).sum(axis=1)
        ar = np.arange(rows)
        eJ, PJ = ev[ar, J], P[ar, J]
        tau = -1.0 + 2.0 * (sumP + np.where(J == 0, 1.0, np.where(PJ >= 0, eJ, 0.0))) + np.where(eJ > 0, eJ, 0.0)
        ess = np.minimum(D / tau, D * math.log10(D))
        out = dict(rhat=np.sqrt(vp / W) if C > 1 else np.full(rows, np.nan), ess=ess, mean=mean,
                   mcse=np.sqrt((A[:, :, 0].sum(axis=1) + N * sb) / (D - 1)) / np.sqrt(ess), n_pairs=J)
    return out


def host_way(samplers, tables, x, split, chunk_rows):
    """predict_bart per chunk of rows (one [chunk x draws] matrix per pooled sampler through the host), the occurrence's series added, the chains cut
    and split, estimator_numpy."""
    n = len(x)
    n0 = min(len(t) for t in tables)
    N = n0 // 2 if split else n0
    out = None
    for r0 in range(0, n, chunk_rows):
        xs = np.asfortranarray(x[r0:r0 + chunk_rows])
        chains = []
        for s, t in zip(samplers, tables):
            z = s.predict_bart(xs) + t[None, :, 0]
            chains += [z[:, :N], z[:, n0 - N:n0]] if split else [z[:, :N]]
        r = estimator_numpy(np.stack(chains, axis=1), len(chains), N)
        if out is None:
            out = {k: np.empty(n, dtype=v.dtype) for k, v in r.items()}
        for k, v in r.items():
            out[k][r0:r0 + len(xs)] = v
    return out


def ar1(phi, n, g):
    s = np.empty(n)
    s[0] = g.standard_normal() / math.sqrt(1.0 - phi * phi)
    for t in range(1, n):
        s[t] = phi * s[t - 1] + g.standard_normal()
    return s


def fmt(ts):
    return f"median {statistics.median(ts) * 1e3:9.2f} ms  (min {min(ts) * 1e3:9.2f}, max {max(ts) * 1e3:9.2f}, {len(ts)} calls)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000, help="training rows of the chain")
    ap.add_argument("--p", type=int, default=51, help="columns of the Friedman design (one goes to the fixed part: p - 1 BART predictors)")
    ap.add_argument("--trees", type=int, default=200)
    ap.add_argument("--burn-in", type=int, default=1000)
    ap.add_argument("--draws", type=int, nargs="+", default=[25, 100], help="kept draws per chain, ascending: one shape each")
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--pool", type=int, default=4, help="chains: times the sampler is pooled with itself")
    ap.add_argument("--sticky", type=float, default=0.0, help="0: a small white series per chain; else the AR(1) coefficient of a series that dominates the trees")
    ap.add_argument("--host-gb", type=float, default=1.0, help="the host way is timed while 8 x rows x pooled draws stays below this")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gap", type=float, default=0.3, help="seconds of rest in front of every timed call, outside the timed window (0: back to back)")
    ap.add_argument("--limit", type=float, default=90.0, help="seconds one timed step may take before the probe gives up")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ppd_probe import new_rows
    from stan4bart_amd import GroupTerm, RRng, generate_friedman_data, make_sampler_args
    from stan4bart_amd._lib import load_library
    from stan4bart_amd.abi import Sampler, StoredSampler
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def write():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    draws = sorted(a.draws)
    d = generate_friedman_data(a.n, ranef=True, causal=True, p=a.p)
    x = d["x"]
    xb = np.asfortranarray(x[:, [j for j in range(a.p) if j != 3]])
    args = make_sampler_args(d["y"], xb, X=np.column_stack([x[:, 3], d["z"]]), groups=[GroupTerm(d["g1"], x[:, 3], "g.1"), GroupTerm(d["g2"], None, "g.2")],
                             iter=a.burn_in + draws[-1], warmup=a.burn_in, keep_fits=False, bart_args={"n.trees": a.trees, "keepTrees": True})
    rng = RRng(99)
    args.seed = int(rng.sample_int(2147483647, 1)[0])
    lib = load_library()
    s = Sampler(lib, "s4b_", args, rng.state)
    held = []
    try:
        t0 = time.perf_counter()
        s.run(a.burn_in, True, 0)
        s.disengage_adaptation()
        by_len, kept = {}, 0
        for n in draws:                                                    # a stored sampler of the first n kept draws per shape
            s.run(n - kept, False, 0)
            kept = n
            by_len[n] = StoredSampler(lib, "s4b_", s.export_bart_state())
            held.append(by_len[n])
        say(f"library {os.environ.get('S4B_LIB_PATH', 'libs4b.so')}; chain: Friedman n={a.n}, {xb.shape[1]} BART predictors, {a.trees} trees, "
            f"{a.burn_in} warm-up + {kept} kept draws in {time.perf_counter() - t0:.1f} s"
            + (f"; every chain carries an AR(1) series of coefficient {a.sticky} that dominates the trees" if a.sticky else ""))
        xn = new_rows(xb, a.rows, 1)
        g = np.random.default_rng(2)
        spread = float(np.std(by_len[draws[0]].predict_bart(np.asfortranarray(xn[:2000]))))
        for n in draws:
            smp, S = by_len[n], n * a.pool
            if a.sticky:
                tables = [(20.0 * spread * math.sqrt(1.0 - a.sticky ** 2) * ar1(a.sticky, n, g))[:, None] for _ in range(a.pool)]
            else:
                tables = [(0.3 * spread * g.standard_normal(n))[:, None] for _ in range(a.pool)]
            pool = dict(dense=np.ones((a.rows, 1)), dense_coef=tables[0], peers=[smp] * (a.pool - 1), peer_dense_coef=tables[1:])
            variants = {CONV: lambda: smp.predict_convergence(xn, **pool), QUANT: lambda: smp.predict_quantiles(xn, (0.025, 0.5, 0.975), **pool)}
            host = 8.0 * a.rows * S <= a.host_gb * 2 ** 30
            if host:
                variants[HOST] = lambda: host_way([smp] * a.pool, tables, xn, True, max(1000, (1 << 27) // (8 * S)))
            res = {k: f() for k, f in variants.items()}                    # warm-up: code objects, allocator, page faults of the outputs
            i, dv = res[CONV]["info"], res[CONV]
            say(f"rows={a.rows}, pooled draws={S} ({a.pool} x {n}), {dv['chains']} chains of {dv['chain_len']} after the split: route {i['route']}, "
                f"{i['chunks']} chunk(s) of {i['rows_per_chunk']} rows, {i['rows_per_sort']} row(s) per workgroup of k_chain_rows at {i['padded_draws']} padded draws, "
                f"{i['launches']} launches, device memory {i['device_bytes'] / 1e6:.1f} MB; the [rows x draws] matrix would be {8e-6 * a.rows * S:.0f} MB")
            npairs = dv["n_pairs"]
            q = np.percentile(npairs, [50, 90, 99])
            say(f"    rhat {np.nanmin(dv['rhat']):.3f} .. {np.nanmax(dv['rhat']):.3f} ({np.mean(dv['rhat'] > 1.01):.2%} of the rows above 1.01), ess "
                f"{np.nanmin(dv['ess']):.1f} .. {np.nanmax(dv['ess']):.1f} (median {np.nanmedian(dv['ess']):.1f}); n_pairs median {q[0]:.0f}, 90 % {q[1]:.0f}, 99 % {q[2]:.0f}, "
                f"max {npairs.max()} (limit {max(0, (dv['chain_len'] - 4) // 2)}); blocks of 64 lags: " + ", ".join(
                    f"{b + 1}: {np.mean(npairs // 32 == b):.2%}" for b in range(int(npairs.max()) // 32 + 1)))
            if host:
                h = res[HOST]
                same = h["n_pairs"] == npairs
                with np.errstate(invalid="ignore"):
                    diff = {k: np.nanmax(np.abs(h[k] - dv[k])[same] / np.maximum(np.abs(dv[k][same]), 1e-300)) for k in ("rhat", "ess", "mean", "mcse")}
                say(f"    (b) vs the device: the same n_pairs in {same.mean():.4%} of the rows; there max relative diff " + ", ".join(f"{k} {v:.2e}" for k, v in diff.items()))
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
            say(f"    predict_convergence / (a) = {med[CONV] / med[QUANT]:.2f}" + (f", (b) / predict_convergence = {med[HOST] / med[CONV]:.2f}" if host else ""))
            write()
    finally:
        for st in held:
            st.free()
        s.free()
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
