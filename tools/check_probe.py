#!/usr/bin/env python3
"""What a posterior predictive check of a finished fit costs on the GPU box: s4b_predict_check (readout_check.inc: per chunk of rows the value
kernel, the fused replicate-and-reduce kernel — Philox, Box-Muller or the uniform, shifted moments to the third, extremes, the weighted histogram
over the thresholds in LDS, the two discrepancy sums — and the fold of the slab partials; once per call the suffix sums, the summary kernel and one
bitonic network over the [(7 + T) x draws] matrix) against
    (floor) predict_ppd with quantiles alone at the same shape: the value kernel, the uploads and the binning of the rows, and the same Philox
            deviates formed once per element (sorted there per row instead of reduced over the rows);
    (bare)  the same call asked for the matrix alone: without the host's statistics of y (`observed`), without k_level_rows and the sort;
    (host)  predict_bart of the rows in row chunks, numpy's deviates and numpy statistics per chunk: sums of powers about a pilot mean, extremes,
            the weights above every threshold and the two discrepancy sums.
Link 1 runs on the same kept trees with an offset that centres z (the replicate is Bernoulli(Phi(z)), T = 0); its floor is the same predict_ppd call.
One stationary chain of the benchmark's Friedman shape supplies the kept trees (tools/spread_probe.py's chain).
    python tools/check_probe.py [--rows 100000] [--draws 100] [--pool 1 4] [--thresholds 0 8 64] [--links 0 1] [--out profiles/predict_check.txt]
The thresholds are evenly spaced quantiles of a sample of the replicate, the weights are uniform on (0, 2).  One warm-up call of each variant, then
the variants alternating with --gap seconds of rest in front of every timed call, medians and min-max.  Wall clock around the calls, which end in a
stream synchronise: binning of the rows on the host, uploads, kernels and downloads are inside for every variant.  The host way draws other deviates,
so its matrix is compared with the device's in distribution only (means over the draws).  Kernel times: run the probe with --device-only --reps 2
--gap 0 and one shape under a kernel trace (the device's own time stamps per launch)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PROBS = (0.025, 0.5, 0.975)
KEY = "predict_check"
FLOOR, HOST = "(floor) predict_ppd, quantiles alone", "(host) predict_bart in row chunks + numpy"
BARE = "predict_check, the matrix alone"
NOISE_KEY = 0x9E3779B97F4A7C15


def new_rows(xb, m, seed):
    g = np.random.default_rng(seed)
    lo, hi = xb.min(axis=0), xb.max(axis=0)
    out = np.empty((m, xb.shape[1]), order="F")
    for j in range(xb.shape[1]):
        out[:, j] = g.uniform(lo[j], hi[j], m)
    return out


def host_way(s, x1, y, w, sigma, th, times, chunk_rows, link, offset):
    """predict_bart per chunk of rows, numpy's deviates, per chunk the weighted sums of powers about a pilot mean (the first chunk's), the extremes,
    the weights above every threshold and the discrepancy sums; the matrix of predict_check (another draw of the noise)."""
    if link:
        from scipy.special import log_ndtr, ndtr          # (the host way of a binary response needs Phi: scipy where it is installed)
    T, W = len(th), w.sum()
    g = np.random.default_rng(5)
    pilot = s1 = s2 = s3 = mn = mx = aw = dr = dob = None
    for r0 in range(0, len(x1), chunk_rows):
        r1 = min(len(x1), r0 + chunk_rows)
        z = s.predict_bart(np.asfortranarray(x1[r0:r1]))
        wc, yc = w[r0:r1], y[r0:r1]
        if link:
            z = z + offset
            v = (g.uniform(size=z.shape) <= ndtr(z)).astype(np.float64)
            lp, lm = log_ndtr(z), log_ndtr(-z)
            t_rep, t_obs = -2.0 * np.where(v > 0.0, lp, lm), -2.0 * np.where(yc[:, None] > 0.0, lp, lm)
        else:
            e = g.standard_normal(z.shape)
            v = z + sigma[None, :] * e
            t_rep, t_obs = e * e, ((yc[:, None] - z) / sigma[None, :]) ** 2
        if pilot is None:
            pilot = (wc @ v) / wc.sum()
            s1, s2, s3, dr, dob = (np.zeros_like(pilot) for _ in range(5))
            mn, mx = np.full_like(pilot, np.inf), np.full_like(pilot, -np.inf)
            aw = np.zeros((T, len(pilot)))
        d = v - pilot
        s1 += wc @ d
        s2 += wc @ (d * d)
        s3 += wc @ (d * d * d)
        dr += wc @ t_rep
        dob += wc @ t_obs
        on = wc > 0.0
        mn, mx = np.minimum(mn, v[on].min(axis=0)), np.maximum(mx, v[on].max(axis=0))
        for j, t in enumerate(th):
            aw[j] += wc @ (v > t)
    m1 = s1 / W
    var = np.maximum(0.0, s2 / W - m1 * m1)
    m3 = s3 / W - 3.0 * m1 * s2 / W + 2.0 * m1 ** 3
    D = np.vstack([pilot + m1, np.sqrt(var), m3, mn, mx, aw / W, dr / W, dob / W])
    D = np.tile(D, (1, times))
    return dict(draws=D, mean=D.mean(axis=1), quantiles=np.quantile(D, PROBS, axis=1))


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
    ap.add_argument("--thresholds", type=int, nargs="+", default=[0, 8, 64], help="T (link 1 runs once, with T = 0)")
    ap.add_argument("--links", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--host-gb", type=float, default=0.5, help="the host way is timed while its chunk matrices (40 x chunk rows x draws) stay below this")
    ap.add_argument("--device-only", action="store_true", help="predict_check alone (for a kernel trace)")
    ap.add_argument("--bin-index", default="auto", choices=("auto", "compare", "search"), help="with --device-only: how the bin is found")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gap", type=float, default=0.2, help="seconds of rest in front of every timed call, outside the timed window (0: back to back)")
    ap.add_argument("--limit", type=float, default=120.0, help="seconds one timed step may take before the probe gives up")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from stan4bart_amd import GroupTerm, RRng, generate_friedman_data, make_sampler_args
    from stan4bart_amd._lib import load_library
    from stan4bart_amd.abi import Sampler
    try:
        import scipy.special  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def write():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def timed(variants):
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
                    sys.exit(1)
        for k in variants:
            say(f"    {k:52s} {fmt(ts[k])}")
        return {k: statistics.median(v) for k, v in ts.items()}
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
        x1 = new_rows(xb, a.rows, 1)
        g = np.random.default_rng(2)
        w = g.uniform(0.0, 2.0, a.rows)
        sig1 = g.uniform(0.8, 1.2, a.draws)
        m = min(a.rows, 2000)
        zs = s.predict_bart(np.asfortranarray(x1[:m]))
        centre = float(zs.mean())
        sample = zs + sig1[None, :] * g.standard_normal(zs.shape)
        for times in a.pool:
            S = a.draws * times
            peers = [s] * (times - 1)
            sigma = np.tile(sig1, times)
            for link in a.links:
                for T in ([0] if link else a.thresholds):
                    th = np.unique(np.quantile(sample, (np.arange(T) + 1.0) / (T + 1.0))) if T else np.zeros(0)
                    assert len(th) == T, "the sample's quantiles coincide: fewer distinct thresholds than asked for"
                    off = np.full(a.rows, -centre) if link else None
                    y = (g.uniform(size=a.rows) < 0.5).astype(np.float64) if link else centre + 5.0 * g.standard_normal(a.rows)

                    def check(how=a.bin_index if a.device_only else "auto", outputs=("mean", "m2", "observed"), probs=PROBS):
                        return s.predict_check(x1, y=y, thresholds=th, probs=probs, outputs=outputs, sigma=None if link else sig1, noise_key=NOISE_KEY, weights=w, peers=peers,
                                               peer_sigma=None if link or times == 1 else [sig1] * (times - 1), offset=off, link=link, bin_index=how)

                    def floor():
                        return s.predict_ppd(x1, probs=PROBS, sigma=sig1, noise_key=NOISE_KEY, peers=peers, peer_sigma=None if times == 1 else [sig1] * (times - 1))
                    variants = {KEY: check}
                    chunk = max(1000, (1 << 26) // (8 * S))
                    if not a.device_only:
                        variants[FLOOR] = floor
                        variants[BARE] = lambda: check(outputs=(), probs=())          # without the host's statistics of y, k_level_rows and the sort
                        if 40.0 * chunk * S <= a.host_gb * 2 ** 30 and (have_scipy or not link):
                            variants[HOST] = lambda: host_way(s, x1, y, w, sigma[:a.draws], th, times, chunk, link, -centre)
                    res = {k: f() for k, f in variants.items()}                    # warm-up: code objects, allocator, page faults of the outputs
                    i = res[KEY]["info"]
                    R = 8 + (T + 1 if T else 0)
                    say(f"rows={a.rows}, pooled draws={S} ({times} x {a.draws}), link {link}, T={T}: route {i['route']}, {i['chunks']} chunk(s) of {i['rows_per_chunk']} rows, "
                        f"{i['launches']} launches, device memory {i['device_bytes'] / 1e6:.1f} MB of which the slab partials "
                        f"{8e-6 * -(-i['rows_per_chunk'] // 128) * R * S:.1f}; the replicate matrix would be {8e-6 * a.rows * S:.0f} MB; posterior mean of the replicate's "
                        f"mean {res[KEY]['mean'][0]:.4f}, sd {res[KEY]['mean'][1]:.4f}, disc_rep {res[KEY]['mean'][5 + T]:.4f}, disc_obs {res[KEY]['mean'][6 + T]:.4f}")
                    if HOST in res:
                        h, p = res[HOST], res[KEY]
                        say("    host (other deviates) vs predict_check, means over the draws: max abs diff " +
                            ", ".join(f"{n} {abs(h['mean'][j] - p['mean'][j]):.2e}" for j, n in enumerate(p["names"]) if not n.startswith("share") or j in (5, 4 + T)))
                    med = timed(variants)
                    if not a.device_only:
                        say("    " + ", ".join(f"predict_check / {k.split(')')[0]}) = {med[KEY] / med[k]:.2f}" for k in (FLOOR, HOST) if k in med))
                    write()
    finally:
        s.free()
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
