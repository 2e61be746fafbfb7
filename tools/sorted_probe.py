#!/usr/bin/env python3
"""What the sorted effects of a finished fit cost on the GPU box: s4b_predict_sorted (readout_sorted.inc: per block of draws the values of ALL rows,
then 8 passes of k_sorted_hist + k_sorted_scan, k_sorted_count, at the end k_sorted_finish and the summary over the draws) against its floor —
predict_quantiles (one arm) / predict_contrast (two arms) with quantiles at the same shape: one walk of the trees and one sort — and against the host
way: predict_bart per arm in row chunks into the [rows x draws] matrix, np.partition along the rows and the counts.  One stationary chain of the
benchmark's Friedman shape supplies the kept trees (tools/quantile_probe.py's chain).
    python tools/sorted_probe.py [--rows 100000] [--draws 100] [--pool 1 4] [--big-rows 1000000] [--out profiles/predict_sorted.txt]
Shapes per pool size (the sampler pooled with itself `pool` times): one arm; two arms on the most used BART predictor; two arms on the least used one.
5 row probs, a top and a bottom tenth (2 cuts), 3 probs over the draws.  Variants: (a) the call, (f) the floor, (c) the host way (only while its
matrix stays below --host-gb).  One warm-up call of each variant, then the variants alternating, medians and min-max.  Wall clock around the calls,
which end in a stream synchronise: binning of the rows on the host, uploads, kernels and downloads are inside for every variant.  The results are
compared before their times are reported.  --big-rows adds one shape of that many rows at pool 1 (a block is 8 draws there), (a) and (f) only.  The
default scratch is a build constant: run the probe again with S4B_LIB_PATH at a library built with -DS4B_SO_SCRATCH_MIB=512 for (d).  --once runs (a)
and (f) a single time each at the first pool (with --big-rows: at the big shape instead) and nothing else: the run to put under a kernel trace."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PROBS = (0.025, 0.5, 0.975)
ROW_PROBS = (0.1, 0.25, 0.5, 0.75, 0.9)
TOP, BOTTOM = (0.1,), (0.1,)


def new_rows(xb, m, seed):
    g = np.random.default_rng(seed)
    lo, hi = xb.min(axis=0), xb.max(axis=0)
    out = np.empty((m, xb.shape[1]), order="F")
    for j in range(xb.shape[1]):
        out[:, j] = g.uniform(lo[j], hi[j], m)
    return out


def host_way(s, x, x0, times, chunk_rows, lo_hi_g, cuts):
    """The way without the entry: predict_bart per arm in row chunks into the full [rows x draws] matrix, np.partition along the rows at the ranks the
    statistics need, the interpolation and the counts."""
    n = len(x)
    parts = []
    for r0 in range(0, n, chunk_rows):
        sl = slice(r0, r0 + chunk_rows)
        v = s.predict_bart(np.asfortranarray(x[sl]))
        if x0 is not None:
            v = v - s.predict_bart(np.asfortranarray(x0[sl]))
        parts.append(v)
    v = np.tile(np.concatenate(parts, axis=0), (1, times))
    ranks = sorted({r for lo, hi, _ in lo_hi_g for r in (lo, hi)} | set(cuts))
    y = np.partition(v, ranks, axis=0)
    srt = np.array([y[lo] + g * (y[hi] - y[lo]) for lo, hi, g in lo_hi_g])
    cut = np.array([y[r] for r in cuts])
    above = np.array([(v > c[None, :]).sum(axis=1) for c in cut], dtype=np.int32)
    below = np.array([(v < c[None, :]).sum(axis=1) for c in cut], dtype=np.int32)
    D = np.concatenate([srt, cut], axis=0)
    return dict(draws=D, mean=D.mean(axis=1), quantiles=np.quantile(D, PROBS, axis=1), n_above=above, n_below=below)


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
    ap.add_argument("--big-rows", type=int, default=0, help="one more shape of this many rows at pool 1, (a) and (f) only")
    ap.add_argument("--pool", type=int, nargs="+", default=[1, 4], help="times the sampler is pooled with itself")
    ap.add_argument("--host-gb", type=float, default=0.5, help="the host way is timed while 8 x rows x pooled draws stays below this")
    ap.add_argument("--only-new", action="store_true")
    ap.add_argument("--once", action="store_true", help="(a) and (f) once each at the first pool, no timing: for a kernel trace")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=float, default=60.0, help="seconds one timed step may take before the probe gives up")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from stan4bart_amd import GroupTerm, RRng, generate_friedman_data, make_sampler_args
    from stan4bart_amd._lib import load_library
    from stan4bart_amd.abi import Sampler, fraction_count
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
        say(f"library {os.environ.get('S4B_LIB_PATH', 'libs4b.so')}; chain: Friedman n={a.n}, {xb.shape[1]} BART predictors, {a.trees} trees, "
            f"{a.burn_in} warm-up + {a.draws} kept draws in {time.perf_counter() - t0:.1f} s")
        var = np.asarray(s.get_kept_trees()["var"])
        used = np.bincount(var[var >= 0], minlength=xb.shape[1])
        most, least = int(np.argmax(used)), int(np.argmin(used))
        say(f"rules per BART predictor over the kept draws: the most used is column {most} ({used[most]}), the least used column {least} ({used[least]})")

        def shape(rows, times, which, host_ok):
            S = a.draws * times
            xa = new_rows(xb, rows, 1)
            x0 = None
            if which != "one arm":
                col = most if which == "two arms, most used predictor" else least
                x0 = xa.copy(order="F")
                x0[:, col] = np.roll(xa[:, col], 1)
            arms = 1 if x0 is None else 2
            kw = dict(peers=[s] * (times - 1))
            call = dict(x_test=xa, x_test0=x0, n_arms=arms, row_probs=ROW_PROBS, top=TOP, bottom=BOTTOM, probs=PROBS, **kw)
            floor = (lambda: s.predict_quantiles(xa, PROBS, **kw)) if arms == 1 else (lambda: s.predict_contrast(xa, x0, probs=PROBS, per_row=False, **kw))
            variants = {"(a) predict_sorted": lambda: s.predict_sorted(**call), "(f) the floor: " + ("predict_quantiles" if arms == 1 else "predict_contrast"): floor}
            if a.once:
                for f in variants.values():
                    f()
                return True
            host = host_ok and not a.only_new and 8.0 * rows * S <= a.host_gb * 2 ** 30
            if host:
                lo_hi_g = []
                for p in ROW_PROBS:
                    h = p * (rows - 1)
                    lo = min(int(np.floor(h)), rows - 1)
                    lo_hi_g.append((lo, min(lo + 1, rows - 1), h - lo))
                m = fraction_count(TOP[0], rows)
                cuts = [rows - m - 1, fraction_count(BOTTOM[0], rows)]
                variants["(c) predict_bart + numpy"] = lambda: host_way(s, xa, x0, times, max(1000, (1 << 27) // (8 * a.draws)), lo_hi_g, cuts)
            res = {k: f() for k, f in variants.items()}                    # warm-up: code objects, allocator, page faults of the outputs
            ka = "(a) predict_sorted"
            i = res[ka]["info"]
            say(f"rows={rows}, pooled draws={S} ({times} x {a.draws}), {which}, {len(ROW_PROBS)} row probs, 2 cuts, {len(PROBS)} probs; a [rows x draws] matrix "
                f"would be {8e-6 * rows * S:.0f} MB")
            say(f"    route {i['route']}, {i['blocks']} block(s) of {i['draws_per_block']} draws, {i['targets']} targets, {i['launches']} launches, "
                f"device memory {i['device_bytes'] / 1e6:.1f} MB")
            if host:
                h, b = res["(c) predict_bart + numpy"], res[ka]
                scale = np.abs(b["draws"]).max()
                say(f"    (c) vs (a): draws max diff {np.max(np.abs(h['draws'] - b['draws'])) / scale:.2e} of the scale; "
                    + ", ".join(f"{k} differs in {np.mean(h[k] != b[k]):.3%}" for k in ("n_above", "n_below")))
            ts = {k: [] for k in variants}
            for _ in range(a.reps):                                        # alternating: drifts of the shared host hit every variant alike
                for k, f in variants.items():
                    t0 = time.perf_counter()
                    f()
                    ts[k].append(time.perf_counter() - t0)
                    if ts[k][-1] > a.limit:
                        say(f"    {k}: a call took {ts[k][-1]:.1f} s, beyond the limit of {a.limit:.0f} s: giving up")
                        return False
            for k in variants:
                say(f"    {k:40s} {fmt(ts[k])}")
            med = {k: statistics.median(v) for k, v in ts.items()}
            kf = list(variants)[1]
            say(f"    (a) / (f) = {med[ka] / med[kf]:.3f}" + (f", (c) / (a) = {med['(c) predict_bart + numpy'] / med[ka]:.1f}" if host else ""))
            write()
            return True
        for times in ([] if a.once and a.big_rows else a.pool[:1] if a.once else a.pool):
            for which in ("one arm", "two arms, most used predictor", "two arms, least used predictor"):
                if not shape(a.rows, times, which, True):
                    write()
                    return 1
        if a.big_rows:
            for which in ("one arm", "two arms, most used predictor"):
                if not shape(a.big_rows, 1, which, False):
                    write()
                    return 1
    finally:
        s.free()
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
