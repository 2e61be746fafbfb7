#!/usr/bin/env python3
"""What per-level averages of a finished fit cost on the GPU box: s4b_predict_groups (dev_groups.inc: the value kernel of a chunk of rows, the
segmented reduction over the rows by level, the fold of the slab partials, the level kernel and one bitonic network over the level matrix) against
the two routes the library offered before, for the same answer:
    (a) ceil(L / 8) predict_summary calls (one arm; one per pooled sampler, it does not pool) or predict_contrast calls (two arms) with 8 indicator
        weight vectors each, then mean, sd, quantiles and P(> 0) of the [L x draws] matrix in numpy.  Every call walks every tree for every row again
        and uploads 8 x rows doubles of weights; beyond --calls-max calls the route is not timed and the probe says so;
    (b) predict_bart of the rows (of both arms) in row chunks and a numpy group-by (np.add.reduceat over the rows sorted by level), while its chunk
        matrices stay below --host-gb; then the same numpy summaries.
One stationary chain of the benchmark's Friedman shape supplies the kept trees (tools/contrast_probe.py's chain).
    python tools/groups_probe.py [--rows 100000] [--draws 100] [--pool 1 4] [--levels 8 500 20000] [--out profiles/predict_groups.txt]
The levels are drawn uniformly and the rows sorted by level.  Two arms: arm 0 is arm 1 with the chain's most used BART column overwritten (its own
values in reverse row order).  Last, L = 1 with w = 1 / rows beside predict_contrast with that one weight vector.  One warm-up call of each variant,
then the variants alternating with --gap seconds of rest in front of every timed call, medians and min-max.  Wall clock around the calls, which end in
a stream synchronise: binning of the rows on the host, uploads, kernels and downloads are inside for every variant.  The results are compared before
their times are reported.  Kernel times: run the probe with --device-only --reps 2 --gap 0 under a kernel trace."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PROBS = (0.025, 0.5, 0.975)
KEY = "predict_groups"
A, B = "(a) calls with indicator weights + numpy", "(b) predict_bart in row chunks + numpy group-by"


def new_rows(xb, m, seed):
    g = np.random.default_rng(seed)
    lo, hi = xb.min(axis=0), xb.max(axis=0)
    out = np.empty((m, xb.shape[1]), order="F")
    for j in range(xb.shape[1]):
        out[:, j] = g.uniform(lo[j], hi[j], m)
    return out


def summarise(avg):
    """mean, sd, quantiles and P(> 0) of an [L x draws] matrix: what the host forms on routes (a) and (b)."""
    return dict(mean=avg.mean(axis=1), sd=avg.std(axis=1, ddof=1), quantiles=np.quantile(avg, PROBS, axis=1), p_above=(avg > 0.0).mean(axis=1))


def indicator_way(s, x1, x0, level, L, count, times):
    """ceil(L / 8) calls with the indicators of 8 levels over their counts as weight vectors."""
    rows, out = len(x1), []
    for l0 in range(0, L, 8):
        n = min(8, L - l0)
        w = np.zeros((n, rows))
        for g in range(n):
            on = level == l0 + g
            w[g, on] = 1.0 / max(1, count[l0 + g])
        if x0 is None:          # predict_summary does not pool: one call per pooled sampler (here the same one, `times` times)
            out.append(np.concatenate([s.predict_summary(x1, weights=w)["average"] for _ in range(times)], axis=0).T)
        else:
            out.append(s.predict_contrast(x1, x0, probs=(), weights=w, per_row=False, peers=[s] * (times - 1))["average"].T)
    return summarise(np.vstack(out))


def host_way(s, x1, x0, start, count, times, chunk_rows):
    """predict_bart per chunk of rows (of both arms), the rows of a level added by np.add.reduceat (the rows are sorted by level)."""
    L, S = len(count), None
    total = None
    for r0 in range(0, len(x1), chunk_rows):
        r1 = min(len(x1), r0 + chunk_rows)
        v = s.predict_bart(np.asfortranarray(x1[r0:r1]))
        if x0 is not None:
            v = v - s.predict_bart(np.asfortranarray(x0[r0:r1]))
        if total is None:
            S, total = v.shape[1], np.zeros((L, v.shape[1]))
        inside = np.flatnonzero((start[:-1] < r1) & (start[1:] > r0))          # the levels with rows in the chunk
        at = np.clip(start[inside], r0, r1) - r0
        total[inside] += np.add.reduceat(v, at, axis=0)
    return summarise(np.tile(total / count[:, None], (1, times)))


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
    ap.add_argument("--levels", type=int, nargs="+", default=[8, 500, 20000])
    ap.add_argument("--calls-max", type=int, default=100, help="route (a) is timed while it needs at most this many calls")
    ap.add_argument("--host-gb", type=float, default=0.5, help="route (b) is timed while its chunk matrices (16 x chunk rows x draws) stay below this")
    ap.add_argument("--device-only", action="store_true", help="predict_groups and the L = 1 pair alone (for a kernel trace)")
    ap.add_argument("--skip-one-level", action="store_true", help="leave the L = 1 pair out")
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
        for times in a.pool:
            S = a.draws * times
            peers = [s] * (times - 1)
            for L in a.levels:
                level = np.sort(g.integers(0, L, a.rows))
                start = np.searchsorted(level, np.arange(L + 1))
                count = np.diff(start)
                if (count == 0).any():
                    say(f"    ({int((count == 0).sum())} of {L} levels drew no row: NaN on every route, left out of the comparison)")
                for arms, arm0 in ((1, None), (2, x0)):
                    def groups():
                        return s.predict_groups(x1, level, L, x_test0=arm0, n_arms=arms, probs=PROBS, threshold=0.0, peers=peers, presorted=True)
                    variants = {KEY: groups}
                    calls = -(-L // 8) * (times if arms == 1 else 1)
                    chunk = max(1000, (1 << 27) // (8 * S))
                    if not a.device_only:
                        if calls <= a.calls_max:
                            variants[A] = lambda: indicator_way(s, x1, arm0, level, L, count, times)
                        if 16.0 * chunk * S <= a.host_gb * 2 ** 30:
                            variants[B] = lambda: host_way(s, x1, arm0, start, count, times, chunk)
                        else:
                            skipped_b = f"    {B}: its chunk matrices (16 x {chunk} rows x {S} draws = {16e-9 * chunk * S:.2f} GB) exceed --host-gb {a.host_gb:g}: not timed"
                    res = {k: f() for k, f in variants.items()}                    # warm-up: code objects, allocator, page faults of the outputs
                    i = res[KEY]["info"]
                    say(f"rows={a.rows}, pooled draws={S} ({times} x {a.draws}), L={L}, {arms} arm(s)" + (f" (column {col}, the most used predictor)" if arms == 2 else "")
                        + f": route {i['route']}, {i['chunks']} chunk(s) of {i['rows_per_chunk']} rows, {i['launches']} launches, {i['edge_levels']} level(s) with edge "
                        f"partials, device memory {i['device_bytes'] / 1e6:.1f} MB of which the level matrix {8e-6 * L * S:.1f}; the [rows x draws] matrix would be {8e-6 * a.rows * S:.0f} MB")
                    ok = count > 0
                    sd = np.sqrt(res[KEY]["m2"] / (S - 1))
                    for k in (A, B):
                        if k in res:
                            say(f"    {k[:3]} vs predict_groups: max abs diff mean {np.max(np.abs(res[k]['mean'] - res[KEY]['mean'])[ok]):.2e}, sd {np.max(np.abs(res[k]['sd'] - sd)[ok]):.2e}, "
                                f"quantiles {np.max(np.abs(res[k]['quantiles'] - res[KEY]['quantiles'])[:, ok]):.2e}, P(> 0) {np.max(np.abs(res[k]['p_above'] - res[KEY]['p_above'])[ok]):.2e}")
                    if B not in variants and not a.device_only:
                        say(skipped_b)
                    if A not in variants and not a.device_only:
                        say(f"    {A}: {calls} calls, beyond --calls-max {a.calls_max}: not timed")
                    med = timed(variants)
                    say("    " + ", ".join(f"{k[:3]} / predict_groups = {med[k] / med[KEY]:.1f}" + (f" ({calls} calls)" if k == A else "") for k in (A, B) if k in med))
                    write()
            if a.skip_one_level:
                continue
            # L = 1 with w = 1 / rows beside predict_contrast with that one weight vector
            w = np.full(a.rows, 1.0 / a.rows)
            one = np.zeros(a.rows, dtype=np.int64)
            pair = {"predict_groups, L = 1, w = 1 / rows, sum": lambda: s.predict_groups(x1, one, 1, x_test0=x0, n_arms=2, statistic="sum", weights=w, peers=peers, presorted=True,
                                                                                         outputs=("draws",)),
                    "predict_contrast, one weight vector": lambda: s.predict_contrast(x1, x0, probs=(), weights=w[None, :], per_row=False, peers=peers)}
            res = {k: f() for k, f in pair.items()}
            ka, kb = list(pair)
            say(f"rows={a.rows}, pooled draws={S}, L = 1, two arms: max abs diff of the {S} sums {np.max(np.abs(res[ka]['draws'][0] - res[kb]['average'][:, 0])):.2e}")
            med = timed(pair)
            say(f"    predict_groups / predict_contrast = {med[ka] / med[kb]:.3f}")
            write()
    finally:
        s.free()
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
