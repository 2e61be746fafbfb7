#!/usr/bin/env python3
"""What the read-out of a finished fit costs on the GPU box: s4b_predict_summary (per-row mean / m2 and per-draw row averages formed on the device,
dev_summary.inc) on each of its two routes against the way to the same numbers without it — predict_bart (the full [rows x draws] matrix from
k_predict, downloaded) plus the numpy reductions.  One stationary chain of the benchmark's Friedman shape supplies the kept trees.
    python tools/predict_probe.py [--rows 100000] [--big-rows 1000000] [--draws 100] [--out profiles/predict_summary.txt]
(a) at --rows: both routes and the old way, alternating, after one warm-up call of each; (b) at --big-rows: the two routes alone (the matrix would
be 8 * big-rows * draws bytes).  Wall clock around the ABI call, which ends in a stream synchronise: binning of the new rows on the host, uploads,
kernels and downloads are inside for every variant.  The results of the variants are compared before their times are reported."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def new_rows(xb, m, seed):
    g = np.random.default_rng(seed)
    lo, hi = xb.min(axis=0), xb.max(axis=0)
    out = np.empty((m, xb.shape[1]), order="F")
    for j in range(xb.shape[1]):
        out[:, j] = g.uniform(lo[j], hi[j], m)
    return out


def old_way(s, x, w):
    m = s.predict_bart(x)                                   # [rows x draws], downloaded
    mean = m.mean(axis=1)
    m2 = ((m - mean[:, None]) ** 2).sum(axis=1)
    return dict(mean=mean, m2=m2, average=(w @ m).T)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append(time.perf_counter() - t0)
    return r, out


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
    ap.add_argument("--big-rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from stan4bart_amd import GroupTerm, RRng, generate_friedman_data, make_sampler_args
    from stan4bart_amd._lib import load_library
    from stan4bart_amd.abi import Sampler
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
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
        say(f"chain: Friedman n={a.n}, {xb.shape[1]} BART predictors, {a.trees} trees, {a.burn_in} warm-up + {a.draws} kept draws in {time.perf_counter() - t0:.1f} s")
        xa = new_rows(xb, a.rows, 1)
        w = np.full((1, a.rows), 1.0 / a.rows)
        variants = {"summary, staged route": lambda: s.predict_summary(xa, weights=w, route="staged"),
                    "summary, global route": lambda: s.predict_summary(xa, weights=w, route="global"),
                    "predict_bart + numpy": lambda: old_way(s, xa, w)}
        res = {k: f() for k, f in variants.items()}                    # warm-up: code objects, allocator, page faults of the outputs
        info = {k: res[k]["info"] for k in list(variants)[:2]}
        say(f"(a) rows={a.rows}, draws={a.draws}: largest draw {info['summary, staged route']['largest_draw_nodes']} nodes; staged: route "
            f"{info['summary, staged route']['route']}, {info['summary, staged route']['staging_bytes']} staging bytes per buffer, "
            f"{info['summary, staged route']['workgroups']} workgroups of {info['summary, staged route']['rows_per_tile']}; device memory of a call "
            f"{info['summary, staged route']['device_bytes'] / 1e6:.1f} MB; the draws matrix alone {8 * a.rows * a.draws / 1e6:.1f} MB")
        old = res["predict_bart + numpy"]
        for k in list(variants)[:2]:
            say(f"    {k} vs predict_bart + numpy: max rel diff mean {np.max(np.abs(res[k]['mean'] - old['mean']) / np.abs(old['mean'])):.2e}, "
                f"m2 {np.max(np.abs(res[k]['m2'] - old['m2']) / old['m2']):.2e}, average {np.max(np.abs(res[k]['average'] - old['average']) / np.abs(old['average'])):.2e}")
        assert np.array_equal(res["summary, staged route"]["mean"], res["summary, global route"]["mean"])
        times = {k: [] for k in variants}
        for _ in range(a.reps):                                        # alternating: drifts of the shared host hit every variant alike
            for k, f in variants.items():
                times[k] += timed(f, 1)[1]
        for k in variants:
            say(f"    {k:24s} {fmt(times[k])}")
        if a.big_rows:
            xbig = new_rows(xb, a.big_rows, 2)
            wb = np.full((1, a.big_rows), 1.0 / a.big_rows)
            big = {"summary, staged route": lambda: s.predict_summary(xbig, weights=wb, route="staged"),
                   "summary, global route": lambda: s.predict_summary(xbig, weights=wb, route="global")}
            r0 = {k: f() for k, f in big.items()}
            say(f"(b) rows={a.big_rows}, draws={a.draws}: device memory of a call {r0['summary, staged route']['info']['device_bytes'] / 1e6:.1f} MB; "
                f"the draws matrix alone would be {8 * a.big_rows * a.draws / 1e6:.1f} MB")
            tb = {k: [] for k in big}
            for _ in range(max(2, a.reps // 2)):
                for k, f in big.items():
                    tb[k] += timed(f, 1)[1]
            for k in big:
                say(f"    {k:24s} {fmt(tb[k])}")
    finally:
        s.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
