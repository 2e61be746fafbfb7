#!/usr/bin/env python3
"""What the across-row spread of the fitted values or the effects of a finished fit costs on the GPU box: s4b_predict_spread (readout_spread.inc: per
chunk of rows the value kernel, the per-draw reduction of the chunk's values — shifted moments, extremes and the weighted histogram over the
thresholds in LDS — and the fold of the slab partials; once per call the suffix sums, the summary kernel and one bitonic network over the
[(4 + 2 T) x draws] matrix) against
    (floor) predict_quantiles (one arm) or predict_contrast (two arms, mean and m2 per row) at the same shape: what the value kernel, the uploads and the
            binning of the rows cost without any reduction over the rows;
    (host)  predict_bart of the rows (of both arms) in row chunks and numpy per chunk: sums, sums of squares about a pilot mean, extremes, and the
            weights and weighted values above every threshold.
At the largest T the two ways of finding a value's bin — a count of compares against the wave-uniform thresholds, and a search through a copy of them
in LDS — are timed side by side (bin_index "compare" / "search"); their results are compared bit for bit first.
One stationary chain of the benchmark's Friedman shape supplies the kept trees (tools/groups_probe.py's chain).
    python tools/spread_probe.py [--rows 100000] [--draws 100] [--pool 1 4] [--thresholds 1 8 64] [--arms 1 2] [--out profiles/predict_spread.txt]
The thresholds are evenly spaced quantiles of a sample of the values, the weights are uniform on (0, 2).  Two arms: arm 0 is arm 1 with the chain's most
used BART column overwritten (its own values in reverse row order).  One warm-up call of each variant, then the variants alternating with --gap seconds
of rest in front of every timed call, medians and min-max.  Wall clock around the calls, which end in a stream synchronise: binning of the rows on the
host, uploads, kernels and downloads are inside for every variant.  The results are compared before their times are reported.  Kernel times: run the
probe with --device-only --reps 2 --gap 0 and one shape under a kernel trace (the device's own time stamps per launch)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PROBS = (0.025, 0.5, 0.975)
KEY = "predict_spread"
FLOOR, HOST = "(floor) predict_quantiles / predict_contrast", "(host) predict_bart in row chunks + numpy"
COMPARE, SEARCH = "predict_spread, bin by compares", "predict_spread, bin by search"


def new_rows(xb, m, seed):
    g = np.random.default_rng(seed)
    lo, hi = xb.min(axis=0), xb.max(axis=0)
    out = np.empty((m, xb.shape[1]), order="F")
    for j in range(xb.shape[1]):
        out[:, j] = g.uniform(lo[j], hi[j], m)
    return out


def host_way(s, x1, x0, w, th, times, chunk_rows):
    """predict_bart per chunk of rows (of both arms); per chunk the weighted sums about a pilot mean (the first chunk's), the extremes and the sums
    above every threshold; the matrix of predict_spread and numpy's summaries."""
    T, W = len(th), w.sum()
    pilot = s1 = s2 = mn = mx = aw = asum = None
    for r0 in range(0, len(x1), chunk_rows):
        r1 = min(len(x1), r0 + chunk_rows)
        v = s.predict_bart(np.asfortranarray(x1[r0:r1]))
        if x0 is not None:
            v = v - s.predict_bart(np.asfortranarray(x0[r0:r1]))
        wc = w[r0:r1]
        if pilot is None:
            pilot = (wc @ v) / wc.sum()
            s1, s2 = np.zeros_like(pilot), np.zeros_like(pilot)
            mn, mx = np.full_like(pilot, np.inf), np.full_like(pilot, -np.inf)
            aw, asum = np.zeros((T, len(pilot))), np.zeros((T, len(pilot)))
        d = v - pilot
        s1 += wc @ d
        s2 += wc @ (d * d)
        on = wc > 0.0
        mn, mx = np.minimum(mn, v[on].min(axis=0)), np.maximum(mx, v[on].max(axis=0))
        wv = wc[:, None] * v
        for j, t in enumerate(th):
            above = v > t
            aw[j] += wc @ above
            asum[j] += (wv * above).sum(axis=0)
    mean = pilot + s1 / W
    sd = np.sqrt(np.maximum(0.0, s2 / W - (s1 / W) ** 2))
    D = np.vstack([mean, sd, mn, mx, aw / W, asum / W])
    D = np.tile(D, (1, times))
    return dict(draws=D, mean=D.mean(axis=1), sd=D.std(axis=1, ddof=1), quantiles=np.quantile(D, PROBS, axis=1))


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
    ap.add_argument("--thresholds", type=int, nargs="+", default=[1, 8, 64], help="T")
    ap.add_argument("--arms", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--host-gb", type=float, default=0.5, help="the host way is timed while its chunk matrices (16 x chunk rows x draws) stay below this")
    ap.add_argument("--device-only", action="store_true", help="predict_spread alone (for a kernel trace)")
    ap.add_argument("--bin-index", default="auto", choices=("auto", "compare", "search"), help="with --device-only: how the bin is found")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gap", type=float, default=0.2, help="seconds of rest in front of every timed call, outside the timed window (0: back to back)")
    ap.add_argument("--limit", type=float, default=120.0, help="seconds one timed step may take before the probe gives up")
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
        trees = s.get_kept_trees()
        rules = np.bincount(trees["var"][trees["var"] >= 0], minlength=xb.shape[1])
        col = int(np.argmax(rules))
        x1 = new_rows(xb, a.rows, 1)
        x0 = x1.copy(order="F")
        x0[:, col] = x1[::-1, col]
        g = np.random.default_rng(2)
        w = g.uniform(0.0, 2.0, a.rows)
        m = min(a.rows, 2000)
        sample = {1: s.predict_bart(np.asfortranarray(x1[:m]))}
        sample[2] = sample[1] - s.predict_bart(np.asfortranarray(x0[:m]))
        for times in a.pool:
            S = a.draws * times
            peers = [s] * (times - 1)
            for T in a.thresholds:
                for arms in a.arms:
                    arm0 = x0 if arms == 2 else None
                    th = np.unique(np.quantile(sample[arms], (np.arange(T) + 1.0) / (T + 1.0)))
                    assert len(th) == T, "the sample's quantiles coincide: fewer distinct thresholds than asked for"

                    def spread(how=a.bin_index if a.device_only else "auto"):
                        return s.predict_spread(x1, th, x_test0=arm0, n_arms=arms, probs=PROBS, weights=w, peers=peers, bin_index=how)

                    def floor():
                        if arms == 1:
                            return s.predict_quantiles(x1, probs=PROBS, peers=peers)
                        return s.predict_contrast(x1, arm0, probs=(), peers=peers)
                    variants = {KEY: spread}
                    chunk = max(1000, (1 << 27) // (8 * S))
                    if not a.device_only:
                        variants[FLOOR] = floor
                        if 16.0 * chunk * S <= a.host_gb * 2 ** 30:
                            variants[HOST] = lambda: host_way(s, x1, arm0, w, th, times, chunk)
                        if T == max(a.thresholds):
                            variants[COMPARE] = lambda: spread("compare")
                            variants[SEARCH] = lambda: spread("search")
                    res = {k: f() for k, f in variants.items()}                    # warm-up: code objects, allocator, page faults of the outputs
                    i = res[KEY]["info"]
                    say(f"rows={a.rows}, pooled draws={S} ({times} x {a.draws}), T={T}, {arms} arm(s)" + (f" (column {col}, the most used predictor)" if arms == 2 else "")
                        + f": route {i['route']}, {i['chunks']} chunk(s) of {i['rows_per_chunk']} rows, {i['launches']} launches, device memory "
                        f"{i['device_bytes'] / 1e6:.1f} MB of which the slab partials {8e-6 * -(-i['rows_per_chunk'] // 128) * (5 + 2 * (T + 1)) * S:.1f}; the [rows x draws] matrix "
                        f"would be {8e-6 * a.rows * S:.0f} MB; posterior mean of the sd over the rows {res[KEY]['mean'][1]:.4f}")
                    if HOST in res:
                        h, p = res[HOST], res[KEY]
                        sd = np.sqrt(p["m2"] / (S - 1))
                        say(f"    host vs predict_spread: max abs diff mean {np.max(np.abs(h['draws'][0] - p['draws'][0])):.2e}, sd {np.max(np.abs(h['draws'][1] - p['draws'][1])):.2e}, "
                            f"min / max {np.max(np.abs(h['draws'][2:4] - p['draws'][2:4])):.2e}, share {np.max(np.abs(h['draws'][4:4 + T] - p['draws'][4:4 + T])):.2e}, "
                            f"part {np.max(np.abs(h['draws'][4 + T:] - p['draws'][4 + T:])):.2e}; over the draws: mean {np.max(np.abs(h['mean'] - p['mean'])):.2e}, "
                            f"sd {np.max(np.abs(h['sd'] - sd)):.2e}, quantiles {np.max(np.abs(h['quantiles'] - p['quantiles'])):.2e}")
                    if COMPARE in res:
                        same = all(np.array_equal(res[COMPARE][k], res[SEARCH][k]) for k in ("draws", "mean", "m2", "quantiles"))
                        say(f"    bin by compares and bin by search: {'the same bits' if same else 'DIFFERENT RESULTS'}")
                    med = timed(variants)
                    if not a.device_only:
                        say("    " + ", ".join(f"predict_spread / {k.split(')')[0]}) = {med[KEY] / med[k]:.2f}" for k in (FLOOR, HOST) if k in med))
                    write()
    finally:
        s.free()
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
