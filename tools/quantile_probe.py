#!/usr/bin/env python3
"""What the per-row credible interval of a finished fit costs on the GPU box: s4b_predict_quantiles (dev_quantile.inc: the values of a chunk of rows,
then one bitonic network per chunk) against what there was before it — predict_bart in row chunks, the linear part added on the host and
np.quantile(axis=1) — which needs nothing of this library's quantile entry (it is the parent commit's way on the parent commit's code).  One
stationary chain of the benchmark's Friedman shape supplies the kept trees (tools/pd_probe.py's chain, DESIGN.md 5.5's shape).
    python tools/quantile_probe.py [--rows 100000] [--draws 100] [--pool 1 4 40] [--scratch-mib 64 256] [--out profiles/predict_quantiles.txt]
Variants per pool size (the sampler pooled with itself `pool` times; the peers get tables of their own): (a) the new call with the library's scratch
limit, (a@N) the new call with scratch_bytes = N MiB, (c) the host way (only while its [rows x draws] matrix stays below --host-gb).  One warm-up call
of each variant, then the variants alternating, medians and min-max.  Wall clock around the calls, which end in a stream synchronise: binning of the
rows on the host, uploads, kernels and downloads are inside for every variant.  The results are compared before their times are reported.  A call
that runs past --limit seconds ends the probe.  A scratch limit ABOVE the library's own needs a build with -DS4B_QT_SCRATCH_MIB=N loaded through
S4B_LIB_PATH: run the probe once more with it (--only-new skips the host way)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PROBS = (0.025, 0.5, 0.975)
KEY_A = "(a) library's scratch limit"


def new_rows(xb, m, seed):
    g = np.random.default_rng(seed)
    lo, hi = xb.min(axis=0), xb.max(axis=0)
    out = np.empty((m, xb.shape[1]), order="F")
    for j in range(xb.shape[1]):
        out[:, j] = g.uniform(lo[j], hi[j], m)
    return out


def host_way(s, x, dense, coefs, chunk_rows):
    """The way there was: per chunk of rows predict_bart (the [chunk x draws] matrix through the host), the same sampler's draws once per table of the
    pool, the linear part added, np.quantile along the draws."""
    out = np.empty((len(PROBS), len(x)))
    for r0 in range(0, len(x), chunk_rows):
        bart = s.predict_bart(np.asfortranarray(x[r0:r0 + chunk_rows]))
        v = np.concatenate([bart + dense[r0:r0 + chunk_rows] @ c.T for c in coefs], axis=1)
        out[:, r0:r0 + chunk_rows] = np.quantile(v, PROBS, axis=1)
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
    ap.add_argument("--pool", type=int, nargs="+", default=[1, 4, 40], help="times the sampler is pooled with itself")
    ap.add_argument("--scratch-mib", type=int, nargs="*", default=[64, 256], help="scratch limits timed beside the library's own")
    ap.add_argument("--host-gb", type=float, default=0.5, help="the host way is timed while 8 x rows x pooled draws stays below this")
    ap.add_argument("--only-new", action="store_true")
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
        say(f"library {os.environ.get('S4B_LIB_PATH', 'libs4b.so')}; chain: Friedman n={a.n}, {xb.shape[1]} BART predictors, {a.trees} trees, "
            f"{a.burn_in} warm-up + {a.draws} kept draws in {time.perf_counter() - t0:.1f} s")
        xa = new_rows(xb, a.rows, 1)
        g = np.random.default_rng(2)
        dense = np.asfortranarray(g.normal(size=(a.rows, 2)))
        for times in a.pool:
            S = a.draws * times
            coefs = [g.normal(size=(a.draws, 2)) for _ in range(times)]
            kw = dict(dense=dense, dense_coef=coefs[0], peers=[s] * (times - 1), peer_dense_coef=coefs[1:])
            variants = {KEY_A: lambda: s.predict_quantiles(xa, PROBS, **kw)}
            for mib in a.scratch_mib:
                variants[f"(a@{mib}) scratch {mib} MiB"] = lambda mib=mib: s.predict_quantiles(xa, PROBS, scratch_bytes=mib << 20, **kw)
            host = not a.only_new and 8.0 * a.rows * S <= a.host_gb * 2 ** 30
            if host:
                variants["(c) predict_bart + np.quantile"] = lambda: dict(quantiles=host_way(s, xa, dense, coefs, max(1000, (1 << 27) // (8 * S))))
            res = {k: f() for k, f in variants.items()}                    # warm-up: code objects, allocator, page faults of the outputs
            first = res[KEY_A]
            say(f"rows={a.rows}, pooled draws={S} ({times} x {a.draws}), {len(PROBS)} probs, 2 dense columns; a [rows x draws] matrix would be {8e-6 * a.rows * S:.0f} MB")
            for k, r in res.items():
                if "info" in r:
                    i = r["info"]
                    say(f"    {k}: route {i['route']}, {i['chunks']} chunk(s) of {i['rows_per_chunk']} rows, {i['rows_per_sort']} row(s) per sort workgroup at "
                        f"{i['padded_draws']} padded draws, {i['launches']} launches, device memory {i['device_bytes'] / 1e6:.1f} MB")
                    assert np.array_equal(r["quantiles"], first["quantiles"]), "the chunking changed the bits"
                else:
                    say(f"    {k} vs (a): max rel diff {np.max(np.abs(r['quantiles'] - first['quantiles']) / np.abs(first['quantiles'])):.2e}")
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
                say(f"    {k:34s} {fmt(ts[k])}")
            if host:
                med = {k: statistics.median(v) for k, v in ts.items()}
                say(f"    (c) / (a) = {med['(c) predict_bart + np.quantile'] / med[KEY_A]:.2f}")
            write()
    finally:
        s.free()
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
