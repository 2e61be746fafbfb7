#!/usr/bin/env python3
"""What the per-row response curves of a finished fit cost on the GPU box: s4b_predict_curves (readout_curves.inc: per chunk of rows the curves over a
grid of one BART predictor, their summaries per (row, grid point), the extremes across the grid) against
    (a) G s4b_predict_quantiles calls with the column overwritten — the device route without this entry; it gives no centred band, no range, no argmax;
    (b) the host way for the full answer: predict_bart per grid point in row chunks, the centring, mean, std, np.quantile, argmax / argmin and the range.
One stationary chain of the benchmark's Friedman shape supplies the kept trees (tools/contrast_probe.py's chain, DESIGN.md 5.5's shape).
    python tools/curves_probe.py [--rows 100000] [--draws 100] [--pool 1 4] [--grid 20] [--out profiles/predict_curves.txt]
The varied predictor is the chain's most used one, then a noise predictor (the least used).  Per pool size, predictor, link and anchor (none, the
first grid point): the call with every output (also with its scratch limited to --scratch-mib), the call with mean and m2 alone (no sort, no k_curve_rows),
(a) and (b) (without an anchor: neither depends on it; (b) under link 0 while its matrix stays below --host-gb, one call, timed as it is).  One warm-up call of each variant, then
the variants alternating with --gap seconds of rest in front of every timed call, medians and min-max.  Wall clock around the calls, which end in a
stream synchronise: binning, uploads, kernels and downloads are inside for every variant.  --device-only runs predict_curves alone, for a kernel trace."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PROBS = (0.025, 0.5, 0.975)
KEY, BARE = "curves, every output", "curves, mean and m2 alone"
DEVICE, HOST = "(a) G predict_quantiles calls", "(b) predict_bart per grid point + numpy"


def new_rows(xb, m, seed):
    g = np.random.default_rng(seed)
    lo, hi = xb.min(axis=0), xb.max(axis=0)
    out = np.empty((m, xb.shape[1]), order="F")
    for j in range(xb.shape[1]):
        out[:, j] = g.uniform(lo[j], hi[j], m)
    return out


def overwritten(x, col, value):
    xg = x.copy(order="F")
    xg[:, col] = value
    return xg


def host_way(s, x, col, grid, times, chunk_rows):
    n, G = len(x), len(grid)
    mean, sd, q = np.empty((n, G)), np.empty((n, G)), np.empty((len(PROBS), n, G))
    p_max, p_min, rng = np.empty((n, G)), np.empty((n, G)), np.empty((len(PROBS), n))
    for r0 in range(0, n, chunk_rows):
        rows = slice(r0, r0 + chunk_rows)
        v = np.stack([np.tile(s.predict_bart(overwritten(x[rows], col, gv)), (1, times)) for gv in grid], axis=1)          # [chunk x G x S]
        mean[rows], sd[rows] = v.mean(axis=2), v.std(axis=2, ddof=1)
        q[:, rows] = np.quantile(v, PROBS, axis=2)
        hi, lo = v.argmax(axis=1), v.argmin(axis=1)
        for g in range(G):
            p_max[rows, g], p_min[rows, g] = (hi == g).mean(axis=1), (lo == g).mean(axis=1)
        rng[:, rows] = np.quantile(v.max(axis=1) - v.min(axis=1), PROBS, axis=1)
    return dict(mean=mean, sd=sd, quantiles=q, p_max=p_max, p_min=p_min, range_quantiles=rng)


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
    ap.add_argument("--pool", type=int, nargs="+", default=[1, 4], help="times the sampler is pooled with itself")
    ap.add_argument("--links", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--host-gb", type=float, default=2.0, help="the host way is timed while 8 x rows x grid x pooled draws stays below this")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gap", type=float, default=0.2, help="seconds of rest in front of every timed call, outside the timed window (0: back to back)")
    ap.add_argument("--limit", type=float, default=60.0, help="seconds one timed step may take before the probe gives up")
    ap.add_argument("--scratch-mib", type=int, nargs="*", default=[], help="also time the call with its value scratch limited to these sizes (below the library's own)")
    ap.add_argument("--device-only", action="store_true", help="predict_curves alone (for a kernel trace)")
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
        trees = s.get_kept_trees()
        rules = np.bincount(trees["var"][trees["var"] >= 0], minlength=xb.shape[1])
        columns = (("most used predictor", int(np.argmax(rules))), ("noise predictor, the least used", int(np.argmin(rules))))
        x1 = new_rows(xb, a.rows, 1)
        for times in a.pool:
            S = a.draws * times
            pool = dict(peers=[s] * (times - 1))          # (no linear parts: they do not move with the grid, and the host way then forms the same numbers)
            for what, col in columns:
                grid = np.quantile(xb[:, col], np.linspace(0.05, 0.95, a.grid))
                for link in a.links:
                    for anchor in (None, 0):
                        kw = dict(anchor=anchor, probs=PROBS, link=link, **pool)
                        variants = {KEY: lambda: s.predict_curves(x1, col, grid, **kw)}
                        for mib in a.scratch_mib:
                            variants[f"curves, every output, scratch {mib} MiB"] = lambda mib=mib: s.predict_curves(x1, col, grid, scratch_bytes=mib << 20, **kw)
                        if not a.device_only:
                            variants[BARE] = lambda: s.predict_curves(x1, col, grid, outputs=("mean", "m2"), **dict(kw, probs=()))
                            if anchor is None:
                                variants[DEVICE] = lambda: [s.predict_quantiles(overwritten(x1, col, gv), PROBS, link=link, **pool) for gv in grid][0]
                                if link == 0 and 8.0 * a.rows * a.grid * S <= a.host_gb * 2 ** 30:
                                    variants[HOST] = lambda: host_way(s, x1, col, grid, times, max(200, (1 << 27) // (8 * S * a.grid)))
                        host_fn = variants.pop(HOST, None)          # the host way takes tens of seconds: one call, timed as it is
                        res = {k: f() for k, f in variants.items()}                    # warm-up: code objects, allocator, page faults of the outputs
                        if host_fn:
                            t0 = time.perf_counter()
                            res[HOST] = host_fn()
                            host_s = time.perf_counter() - t0
                        i = res[KEY]["info"]
                        say(f"rows={a.rows}, G={a.grid}, pooled draws={S} ({times} x {a.draws}), link {link}, anchor {anchor}, column {col} ({what}: {rules[col]} rules in "
                            f"{a.draws} draws): route {i['route']}, affected trees at most {i['largest_affected']} of {a.trees} per draw, {i['total_affected'] / S:.1f} on "
                            f"average; {i['chunks']} chunk(s) of {i['rows_per_chunk']} rows, {i['launches']} launches, device memory {i['device_bytes'] / 1e6:.1f} MB; G "
                            f"[rows x draws] matrices would be {8e-6 * a.rows * S * a.grid:.0f} MB")
                        if HOST in res:
                            h = res[HOST]
                            say(f"    (b) vs the call: max abs diff mean {np.max(np.abs(h['mean'] - res[KEY]['mean'])):.2e}, quantiles "
                                f"{np.max(np.abs(h['quantiles'] - res[KEY]['quantiles'])):.2e}, p_max {np.max(np.abs(h['p_max'] - res[KEY]['p_max'])):.2e}, range quantiles "
                                f"{np.max(np.abs(h['range_quantiles'] - res[KEY]['range_quantiles'])):.2e}")
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
                            say(f"    {k:42s} {fmt(ts[k])}")
                        med = {k: statistics.median(v) for k, v in ts.items()}
                        if host_fn:
                            med[HOST] = host_s
                            say(f"    {HOST:42s} one call {host_s * 1e3:9.2f} ms")
                        if DEVICE in med:
                            say("    " + ", ".join(f"{k.split(')')[0]}) / call = {med[k] / med[KEY]:.2f}" for k in (DEVICE, HOST) if k in med))
                        write()
    finally:
        s.free()
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
