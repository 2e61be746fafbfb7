#!/usr/bin/env python3
"""What the per-row description of a finished fit costs on the GPU box: s4b_predict_describe (readout_describe.inc: the values of a chunk of rows, then
k_row_describe — one bitonic network per chunk, the windows, the counts and, with the MAD, a second network) against its floor — predict_quantiles
(one arm) / predict_contrast (two arms) at the same shape: the value kernel and one sort — and against the host way: predict_bart in row chunks, the
linear part added on the host, numpy's sort and the same statistics.  One stationary chain of the benchmark's Friedman shape supplies the kept trees
(tools/quantile_probe.py's chain).
    python tools/describe_probe.py [--rows 100000] [--draws 100] [--pool 1 4] [--arms 1 2] [--out profiles/predict_describe.txt]
Variants per pool size (the sampler pooled with itself `pool` times; the peers get tables of their own) and number of arms: (a) everything but the MAD,
(b) everything, (f) the floor, (c) the host way (only while its [rows x draws] matrix stays below --host-gb).  One warm-up call of each variant, then
the variants alternating, medians and min-max.  Wall clock around the calls, which end in a stream synchronise: binning of the rows on the host,
uploads, kernels and downloads are inside for every variant.  The results are compared before their times are reported.  A call that runs past --limit
seconds ends the probe.  --once runs (a), (b) and (f) a single time each, in this order, and nothing else: the run to put under a kernel trace."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PROBS = (0.025, 0.5, 0.975)
NO_MAD = ("quantiles", "median", "hdi", "hdi_start", "n_above", "n_below")


def new_rows(xb, m, seed):
    g = np.random.default_rng(seed)
    lo, hi = xb.min(axis=0), xb.max(axis=0)
    out = np.empty((m, xb.shape[1]), order="F")
    for j in range(xb.shape[1]):
        out[:, j] = g.uniform(lo[j], hi[j], m)
    return out


def host_way(s, x, x0, dense, coefs, chunk_rows, counts, thresholds):
    """The way without the entry: per chunk of rows predict_bart (the [chunk x draws] matrix through the host; two arms: twice), the same sampler's draws
    once per table of the pool, the linear part added, np.sort along the draws and the statistics of the sorted rows."""
    n, T = len(x), len(thresholds)
    out = dict(quantiles=np.empty((len(PROBS), n)), median=np.empty(n), mad=np.empty(n), hdi=np.empty((len(counts), 2, n)),
               hdi_start=np.empty((len(counts), n), dtype=np.int32), n_above=np.empty((T, n), dtype=np.int32), n_below=np.empty((T, n), dtype=np.int32))
    for r0 in range(0, n, chunk_rows):
        sl = slice(r0, r0 + chunk_rows)
        bart = s.predict_bart(np.asfortranarray(x[sl]))
        if x0 is None:
            v = np.concatenate([bart + dense[sl] @ c.T for c in coefs], axis=1)
        else:          # (the shared dense part cancels)
            v = np.tile(bart - s.predict_bart(np.asfortranarray(x0[sl])), (1, len(coefs)))
        xs = np.sort(v, axis=1)
        S, rows = xs.shape[1], np.arange(xs.shape[0])
        out["quantiles"][:, sl] = np.quantile(xs, PROBS, axis=1)
        med = np.median(xs, axis=1)
        out["median"][sl] = med
        out["mad"][sl] = np.median(np.abs(xs - med[:, None]), axis=1)
        for c, m in enumerate(counts):
            j = np.argmin(xs[:, m - 1:] - xs[:, :S - m + 1], axis=1)
            out["hdi_start"][c, sl] = j
            out["hdi"][c, 0, sl], out["hdi"][c, 1, sl] = xs[rows, j], xs[rows, j + m - 1]
        for t, th in enumerate(thresholds):
            out["n_above"][t, sl] = (xs > th).sum(axis=1)
            out["n_below"][t, sl] = (xs < th).sum(axis=1)
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
    ap.add_argument("--arms", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--host-gb", type=float, default=0.5, help="the host way is timed while 8 x rows x pooled draws stays below this")
    ap.add_argument("--only-new", action="store_true")
    ap.add_argument("--once", action="store_true", help="(a), (b) and (f) once each, no timing: for a kernel trace")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=float, default=60.0, help="seconds one timed step may take before the probe gives up")
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
    xb = np.asfortranarray(np.column_stack([x[:, [j for j in range(a.p) if j != 3]], np.asarray(d["z"], dtype=np.float64)]))
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
        say(f"library {os.environ.get('S4B_LIB_PATH', 'libs4b.so')}; chain: Friedman n={a.n}, {xb.shape[1]} BART predictors (the last one the treatment), "
            f"{a.trees} trees, {a.burn_in} warm-up + {a.draws} kept draws in {time.perf_counter() - t0:.1f} s")
        xa = new_rows(xb, a.rows, 1)
        treat = xb.shape[1] - 1
        x1, x0 = xa.copy(order="F"), xa.copy(order="F")
        x1[:, treat], x0[:, treat] = 1.0, 0.0
        g = np.random.default_rng(2)
        dense = np.asfortranarray(g.normal(size=(a.rows, 2)))
        for times in a.pool:
            S = a.draws * times
            coefs = [g.normal(size=(a.draws, 2)) for _ in range(times)]
            counts = [math.ceil(0.5 * S), math.ceil(0.95 * S)]
            for arms in a.arms:
                kw = dict(dense=dense, dense_coef=coefs[0], peers=[s] * (times - 1), peer_dense_coef=coefs[1:])
                rows1, rows0 = (xa, None) if arms == 1 else (x1, x0)
                thresholds = (0.0,) if arms == 2 else (float(np.median(d["y"])),)
                thresholds += (thresholds[0] - 0.1, thresholds[0] + 0.1)
                call = dict(x_test=rows1, x_test0=rows0, n_arms=arms, hdi_count=counts, thresholds=thresholds, probs=PROBS, **kw)
                floor = (lambda: s.predict_quantiles(rows1, PROBS, **kw)) if arms == 1 else (lambda: s.predict_contrast(rows1, rows0, probs=PROBS, per_row=False, **kw))
                variants = {"(a) describe without the MAD": lambda: s.predict_describe(outputs=NO_MAD, **call),
                            "(b) describe with the MAD": lambda: s.predict_describe(**call),
                            "(f) the floor: " + ("predict_quantiles" if arms == 1 else "predict_contrast"): floor}
                if a.once:
                    for k in variants:          # (a), (b), (f) in this order: the dispatches of k_row_describe are (a)'s, then (b)'s
                        variants[k]()
                    continue
                host = not a.only_new and 8.0 * a.rows * S <= a.host_gb * 2 ** 30
                if host:
                    variants["(c) predict_bart + numpy"] = lambda: host_way(s, rows1, rows0, dense, coefs, max(1000, (1 << 27) // (8 * S)), counts, thresholds)
                res = {k: f() for k, f in variants.items()}                    # warm-up: code objects, allocator, page faults of the outputs
                ka, kb, kf = list(variants)[:3]
                i = res[kb]["info"]
                say(f"rows={a.rows}, pooled draws={S} ({times} x {a.draws}), {arms} arm(s), {len(PROBS)} probs, {len(counts)} windows, {len(thresholds)} thresholds, "
                    f"2 dense columns; a [rows x draws] matrix would be {8e-6 * a.rows * S:.0f} MB")
                say(f"    route {i['route']}, {i['chunks']} chunk(s) of {i['rows_per_chunk']} rows, {i['rows_per_sort']} row(s) per sort workgroup at "
                    f"{i['padded_draws']} padded draws, {i['sort_lds_bytes']} bytes of LDS, {i['launches']} launches, device memory {i['device_bytes'] / 1e6:.1f} MB")
                assert np.array_equal(res[ka]["quantiles"], res[kf]["quantiles"]) and np.array_equal(res[kb]["quantiles"], res[kf]["quantiles"]), "the quantiles are not the floor's"
                assert all(np.array_equal(res[ka][k], res[kb][k]) for k in NO_MAD), "the MAD changed another output"
                if host:
                    h, b = res["(c) predict_bart + numpy"], res[kb]
                    scale = np.abs(b["quantiles"]).max()
                    say("    (c) vs (b): " + ", ".join(f"{k} max diff {np.max(np.abs(h[k] - b[k])) / scale:.2e} of the scale" for k in ("quantiles", "median", "mad", "hdi")) +
                        "; " + ", ".join(f"{k} differs in {np.mean(h[k] != b[k]):.2%}" for k in ("hdi_start", "n_above", "n_below")))
                ts = {k: [] for k in variants}
                for _ in range(a.reps):                                        # alternating: drifts of the shared host hit every variant alike
                    for k, f in variants.items():
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
                say(f"    (a) / (f) = {med[ka] / med[kf]:.3f}, (b) / (a) = {med[kb] / med[ka]:.3f}" + (f", (c) / (b) = {med['(c) predict_bart + numpy'] / med[kb]:.1f}" if host else ""))
                write()
    finally:
        s.free()
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
