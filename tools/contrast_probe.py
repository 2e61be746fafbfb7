#!/usr/bin/env python3
"""What the per-row treatment effect of a finished fit costs on the GPU box: s4b_predict_contrast (dev_contrast.inc: the paired differences of a chunk
of rows over the affected trees alone, their row and draw summaries, one bitonic network per chunk) against
    (a) two s4b_predict_quantiles calls over the two arms — what walking both arms in full costs on the device, though it cannot give the answer
        (quantiles of two correlated columns do not subtract);
    (b) the host way: predict_bart of both arms in row chunks, the difference, then mean, std and np.quantile along the draws.
One stationary chain of the benchmark's Friedman shape supplies the kept trees (tools/quantile_probe.py's chain, DESIGN.md 5.5's shape).
    python tools/contrast_probe.py [--rows 100000] [--draws 100] [--pool 1 4] [--out profiles/predict_contrast.txt]
Arm 0 is arm 1 with ONE BART column overwritten (its own values in reverse row order): the chain's most used predictor, then its least used one.  Two
dense columns are shared by the arms (under link 0 the contrast does not evaluate them; (a) does).  Per pool size, column and link: the contrast with
quantiles, mean / m2 and one weight vector; the same without quantiles; (a); (b) (link 0, while its matrices stay below --host-gb).  One warm-up call
of each variant, then the variants alternating with --gap seconds of rest in front of every timed call (a call that follows another one at once is
measured some 8 ms longer about every other time, whichever variant it is: the call before has just handed 90 MB back to the device's allocator),
medians and min-max.  Wall clock around the calls, which end in a stream synchronise: binning of the
rows on the host, uploads, kernels and downloads are inside for every variant.  The results are compared before their times are reported."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PROBS = (0.025, 0.5, 0.975)
KEY = "contrast: mean, m2, average, quantiles"


def new_rows(xb, m, seed):
    g = np.random.default_rng(seed)
    lo, hi = xb.min(axis=0), xb.max(axis=0)
    out = np.empty((m, xb.shape[1]), order="F")
    for j in range(xb.shape[1]):
        out[:, j] = g.uniform(lo[j], hi[j], m)
    return out


def host_way(s, x1, x0, times, chunk_rows):
    """predict_bart of both arms per chunk of rows (two [chunk x draws] matrices through the host), the same sampler's draws once per member of the
    pool, the difference, mean, std and quantiles along the draws.  The shared linear parts cancel and are left out, as a user would leave them out."""
    n = len(x1)
    mean, sd, q = np.empty(n), np.empty(n), np.empty((len(PROBS), n))
    for r0 in range(0, n, chunk_rows):
        d = s.predict_bart(np.asfortranarray(x1[r0:r0 + chunk_rows])) - s.predict_bart(np.asfortranarray(x0[r0:r0 + chunk_rows]))
        d = np.tile(d, (1, times))
        mean[r0:r0 + chunk_rows], sd[r0:r0 + chunk_rows] = d.mean(axis=1), d.std(axis=1, ddof=1)
        q[:, r0:r0 + chunk_rows] = np.quantile(d, PROBS, axis=1)
    return dict(mean=mean, sd=sd, quantiles=q)


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
    ap.add_argument("--links", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--host-gb", type=float, default=0.5, help="the host way is timed while 16 x rows x pooled draws stays below this")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gap", type=float, default=0.3, help="seconds of rest in front of every timed call, outside the timed window (0: back to back)")
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
        say(f"library {os.environ.get('S4B_LIB_PATH', 'libs4b.so')}; chain: Friedman n={a.n}, {xb.shape[1]} BART predictors, {a.trees} trees, "
            f"{a.burn_in} warm-up + {a.draws} kept draws in {time.perf_counter() - t0:.1f} s")
        trees = s.get_kept_trees()
        rules = np.bincount(trees["var"][trees["var"] >= 0], minlength=xb.shape[1])
        columns = (("most used predictor", int(np.argmax(rules))), ("least used predictor", int(np.argmin(rules))))
        x1 = new_rows(xb, a.rows, 1)
        g = np.random.default_rng(2)
        dense = np.asfortranarray(g.normal(size=(a.rows, 2)))
        w = np.full((1, a.rows), 1.0 / a.rows)
        for times in a.pool:
            S = a.draws * times
            coefs = [g.normal(size=(a.draws, 2)) for _ in range(times)]
            pool = dict(dense=dense, dense_coef=coefs[0], peers=[s] * (times - 1), peer_dense_coef=coefs[1:])
            for what, col in columns:
                x0 = x1.copy(order="F")
                x0[:, col] = x1[::-1, col]
                for link in a.links:
                    variants = {KEY: lambda: s.predict_contrast(x1, x0, probs=PROBS, weights=w, link=link, **pool),
                                "contrast: mean, m2, average": lambda: s.predict_contrast(x1, x0, probs=(), weights=w, link=link, **pool),
                                "(a) two predict_quantiles calls": lambda: (s.predict_quantiles(x1, PROBS, link=link, **pool), s.predict_quantiles(x0, PROBS, link=link, **pool))[0]}
                    host = link == 0 and 16.0 * a.rows * S <= a.host_gb * 2 ** 30
                    if host:
                        variants["(b) predict_bart x 2 + numpy"] = lambda: host_way(s, x1, x0, times, max(1000, (1 << 27) // (8 * S)))
                    res = {k: f() for k, f in variants.items()}                    # warm-up: code objects, allocator, page faults of the outputs
                    i = res[KEY]["info"]
                    say(f"rows={a.rows}, pooled draws={S} ({times} x {a.draws}), link {link}, column {col} ({what}: {rules[col]} rules in {a.draws} draws): route {i['route']}, "
                        f"affected trees at most {i['largest_affected']} of {a.trees} per draw, {i['total_affected'] / S:.1f} on average; {i['chunks']} chunk(s) of "
                        f"{i['rows_per_chunk']} rows, {i['launches']} launches, device memory {i['device_bytes'] / 1e6:.1f} MB; two [rows x draws] matrices would be {16e-6 * a.rows * S:.0f} MB")
                    assert np.array_equal(res[KEY]["mean"], res["contrast: mean, m2, average"]["mean"])
                    if host:
                        sd = np.sqrt(res[KEY]["m2"] / (S - 1))
                        say(f"    (b) vs the contrast: max abs diff mean {np.max(np.abs(res['(b) predict_bart x 2 + numpy']['mean'] - res[KEY]['mean'])):.2e}, sd "
                            f"{np.max(np.abs(res['(b) predict_bart x 2 + numpy']['sd'] - sd)):.2e}, quantiles {np.max(np.abs(res['(b) predict_bart x 2 + numpy']['quantiles'] - res[KEY]['quantiles'])):.2e}")
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
                    say(f"    (a) / contrast = {med['(a) two predict_quantiles calls'] / med[KEY]:.2f}" + (f", (b) / contrast = {med['(b) predict_bart x 2 + numpy'] / med[KEY]:.2f}" if host else ""))
                    write()
    finally:
        s.free()
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
