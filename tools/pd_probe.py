#!/usr/bin/env python3
"""What the partial dependence of a finished fit costs on the GPU box: s4b_partial_dependence (one fused call for all grid points, dev_pd.inc) on each
of its two routes against what there was before it — one predict_summary call per grid value with the column overwritten.  One stationary chain of the
benchmark's Friedman shape supplies the kept trees (DESIGN.md 5.5's shape).
    python tools/pd_probe.py [--rows 100000] [--draws 100] [--grid 20] [--out profiles/partial_dependence.txt]
Run once for an active predictor of the Friedman function and once for a noise predictor (chosen from the kept trees: the most and the fewest
affected trees).  Per predictor: one warm-up call of each variant, then the variants alternating, medians.  Wall clock around the ABI call(s), which
end in a stream synchronise: binning of the rows on the host, uploads, kernels and downloads are inside for every variant.  The results of the
variants are compared before their times are reported.  A variant's call that runs past --limit seconds ends the probe."""
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


def loop_of_summaries(s, x, v, grid, w):
    """The parent's way: per grid value the column overwritten and one predict_summary call (re-binned, re-uploaded, all T trees walked)."""
    xg = np.array(x, order="F")
    cols = []
    for c in grid:
        xg[:, v] = c
        cols.append(s.predict_summary(xg, weights=w)["average"][:, 0])
    return dict(pd=np.column_stack(cols))


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
    ap.add_argument("--grid", type=int, default=20)
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
        kept = s.get_kept_trees()
        rule = kept["var"] >= 0
        per_tree = np.unique(np.column_stack([kept["var"][rule], kept["sample"][rule], kept["tree"][rule]]), axis=0)          # (predictor, draw, tree) once each
        affected = np.bincount(per_tree[:, 0], minlength=xb.shape[1])
        say(f"trees with a rule on a predictor, mean per draw: most {affected.max() / a.draws:.1f} (predictor {int(affected.argmax())}), "
            f"fewest {affected.min() / a.draws:.1f} (predictor {int(affected.argmin())}), over all predictors {affected.mean() / a.draws:.1f}; "
            f"{rule.sum() / a.draws / a.trees:.2f} rules per tree")
        xa = new_rows(xb, a.rows, 1)
        w = np.full((1, a.rows), 1.0 / a.rows)
        for label, v in (("active predictor", int(affected.argmax())), ("noise predictor", int(affected.argmin()))):
            grid = np.quantile(xa[:, v], np.linspace(0.05, 0.95, a.grid))
            variants = {"(a) fused, staged route": lambda: s.partial_dependence(xa, v, grid, route="staged"),
                        "(b) fused, global route": lambda: s.partial_dependence(xa, v, grid, route="global"),
                        f"(c) {a.grid} x predict_summary": lambda: loop_of_summaries(s, xa, v, grid, w)}
            res = {k: f() for k, f in variants.items()}                    # warm-up: code objects, allocator, page faults of the outputs
            info = res["(a) fused, staged route"]["info"]
            A_mean, A_max = info["total_affected"] / a.draws, info["largest_affected"]
            say(f"{label} {v}: rows={a.rows}, draws={a.draws}, G={a.grid}; affected trees per draw: mean {A_mean:.1f}, largest {A_max} of {a.trees}; "
                f"walks per (row, draw): fused T + G A = {a.trees + a.grid * A_mean:.0f}, loop G T = {a.grid * a.trees} (ratio {a.grid * a.trees / (a.trees + a.grid * A_mean):.1f}); "
                f"staged: route {info['route']}, {info['staging_bytes']} staging bytes per buffer, {info['workgroups']} workgroups of {info['rows_per_tile']}; "
                f"device memory of a fused call {info['device_bytes'] / 1e6:.1f} MB")
            old = res[f"(c) {a.grid} x predict_summary"]["pd"]
            for k in list(variants)[:2]:
                say(f"    {k} vs (c): max rel diff {np.max(np.abs(res[k]['pd'] - old) / np.abs(old)):.2e}")
            assert np.array_equal(res["(a) fused, staged route"]["pd"], res["(b) fused, global route"]["pd"])
            times = {k: [] for k in variants}
            for _ in range(a.reps):                                        # alternating: drifts of the shared host hit every variant alike
                for k, f in variants.items():
                    t0 = time.perf_counter()
                    f()
                    times[k].append(time.perf_counter() - t0)
                    if times[k][-1] > a.limit:
                        say(f"    {k}: a call took {times[k][-1]:.1f} s, beyond the limit of {a.limit:.0f} s: giving up")
                        write()
                        return 1
            for k in variants:
                say(f"    {k:28s} {fmt(times[k])}")
            med = {k: statistics.median(ts) for k, ts in times.items()}
            c = f"(c) {a.grid} x predict_summary"
            best = min(("(a) fused, staged route", "(b) fused, global route"), key=med.get)
            say(f"    (c) / (a) = {med[c] / med['(a) fused, staged route']:.2f}, (c) / (b) = {med[c] / med['(b) fused, global route']:.2f}; "
                f"fastest single run of (c) {min(times[c]) * 1e3:.2f} ms against the median of {best[:3]} {med[best] * 1e3:.2f} ms")
    finally:
        s.free()
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
