#!/usr/bin/env python3
"""What projecting the fitted values or the effects of a finished fit on a design costs on the GPU box: s4b_predict_projection
(readout_projection.inc: per chunk of rows the value kernel, the skinny product A' W X of the chunk's values and the fold of the slab partials; once
per call the same for the design's own moments, the Cholesky solve per draw, the summary kernel and one bitonic network over the [(K + 1) x draws]
matrix) against
    (floor) predict_quantiles (one arm) or predict_contrast (two arms, mean and m2 per row) at the same shape: what the value kernel, the uploads and the
            binning of the rows cost without any projection;
    (host)  predict_bart of the rows (of both arms) in row chunks, A.T @ (w * x) per chunk, a numpy Cholesky solve, and numpy's summaries.
One stationary chain of the benchmark's Friedman shape supplies the kept trees (tools/groups_probe.py's chain).
    python tools/projection_probe.py [--rows 100000] [--draws 100] [--pool 1 4] [--columns 8 32] [--arms 1 2] [--out profiles/predict_projection.txt]
The design is an intercept beside standard normal columns, the weights are uniform on (0, 2).  Two arms: arm 0 is arm 1 with the chain's most used
BART column overwritten (its own values in reverse row order).  One warm-up call of each variant, then the variants alternating with --gap seconds of
rest in front of every timed call, medians and min-max.  Wall clock around the calls, which end in a stream synchronise: binning of the rows on the
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
KEY = "predict_projection"
FLOOR, HOST = "(floor) predict_quantiles / predict_contrast", "(host) predict_bart in row chunks + numpy"


def new_rows(xb, m, seed):
    g = np.random.default_rng(seed)
    lo, hi = xb.min(axis=0), xb.max(axis=0)
    out = np.empty((m, xb.shape[1]), order="F")
    for j in range(xb.shape[1]):
        out[:, j] = g.uniform(lo[j], hi[j], m)
    return out


def host_way(s, x1, x0, A, w, times, chunk_rows):
    """predict_bart per chunk of rows (of both arms), the moments added chunk by chunk, the normal equations solved by numpy."""
    WA = w[:, None] * A
    G = A.T @ WA
    b = sm = t = None
    for r0 in range(0, len(x1), chunk_rows):
        r1 = min(len(x1), r0 + chunk_rows)
        v = s.predict_bart(np.asfortranarray(x1[r0:r1]))
        if x0 is not None:
            v = v - s.predict_bart(np.asfortranarray(x0[r0:r1]))
        pb, ps, pt = WA[r0:r1].T @ v, w[r0:r1] @ v, w[r0:r1] @ (v * v)
        b, sm, t = (pb, ps, pt) if b is None else (b + pb, sm + ps, t + pt)
    b, sm, t = (np.tile(q, (1, times)) if q.ndim == 2 else np.tile(q, times) for q in (b, sm, t))
    L = np.linalg.cholesky(G)
    beta = np.linalg.solve(L.T, np.linalg.solve(L, b))
    r2 = 1.0 - (t - (beta * b).sum(axis=0)) / (t - sm * sm / w.sum())
    M = np.vstack([beta, r2[None, :]])
    return dict(coef=beta, r2=r2, mean=M.mean(axis=1), sd=M.std(axis=1, ddof=1), quantiles=np.quantile(M, PROBS, axis=1).T, p_above=(M > 0.0).mean(axis=1))


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
    ap.add_argument("--columns", type=int, nargs="+", default=[8, 32], help="design columns, the intercept included")
    ap.add_argument("--arms", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--host-gb", type=float, default=0.5, help="the host way is timed while its chunk matrices (16 x chunk rows x draws) stay below this")
    ap.add_argument("--device-only", action="store_true", help="predict_projection alone (for a kernel trace)")
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
        for times in a.pool:
            S = a.draws * times
            peers = [s] * (times - 1)
            for K in a.columns:
                A = g.standard_normal((a.rows, K))
                A[:, 0] = 1.0
                for arms in a.arms:
                    arm0 = x0 if arms == 2 else None

                    def projection():
                        return s.predict_projection(x1, A, x_test0=arm0, n_arms=arms, probs=PROBS, threshold=0.0, weights=w, peers=peers)

                    def floor():
                        if arms == 1:
                            return s.predict_quantiles(x1, probs=PROBS, peers=peers)
                        return s.predict_contrast(x1, arm0, probs=(), peers=peers)
                    variants = {KEY: projection}
                    chunk = max(1000, (1 << 27) // (8 * S))
                    if not a.device_only:
                        variants[FLOOR] = floor
                        if 16.0 * chunk * S <= a.host_gb * 2 ** 30:
                            variants[HOST] = lambda: host_way(s, x1, arm0, A, w, times, chunk)
                    res = {k: f() for k, f in variants.items()}                    # warm-up: code objects, allocator, page faults of the outputs
                    i = res[KEY]["info"]
                    say(f"rows={a.rows}, pooled draws={S} ({times} x {a.draws}), K={K}, {arms} arm(s)" + (f" (column {col}, the most used predictor)" if arms == 2 else "")
                        + f": route {i['route']}, {i['chunks']} chunk(s) of {i['rows_per_chunk']} rows, {i['launches']} launches, deficient {i['deficient']}, device memory "
                        f"{i['device_bytes'] / 1e6:.1f} MB of which the padded design {8e-6 * a.rows * (8 if K <= 8 else 16 if K <= 16 else 32):.1f}; the [rows x draws] matrix would be "
                        f"{8e-6 * a.rows * S:.0f} MB; mean r2 {res[KEY]['mean'][K]:.4f}")
                    if HOST in res:
                        h, p = res[HOST], res[KEY]
                        sd = np.sqrt(p["m2"] / (S - 1))
                        say(f"    host vs predict_projection: max abs diff coef {np.max(np.abs(h['coef'] - p['coef'])):.2e}, r2 {np.max(np.abs(h['r2'] - p['r2'])):.2e}, "
                            f"mean {np.max(np.abs(h['mean'] - p['mean'])):.2e}, sd {np.max(np.abs(h['sd'] - sd)):.2e}, quantiles {np.max(np.abs(h['quantiles'].T - p['quantiles'])):.2e}, "
                            f"P(> 0) {np.max(np.abs(h['p_above'] - p['p_above'])):.2e}")
                    med = timed(variants)
                    if not a.device_only:
                        say("    " + ", ".join(f"predict_projection / {k.split(')')[0]}) = {med[KEY] / med[k]:.2f}" for k in (FLOOR, HOST) if k in med))
                    write()
    finally:
        s.free()
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
