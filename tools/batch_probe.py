"""Aggregate Gibbs iterations per second of C concurrent chains (host threads, one sampler each) with and without a sweep group
(stan4bart(batch_chains=True) underneath), C = 1, 2, 4, 8, 16, at two shapes: the IHDP shape (stan4bart_amd.cases.ihdp_case: binary,
treatment counterfactual, 75 trees, n = 747) and a Gaussian fit with random effects at n = 4 096 (the largest solo sweep).  The batched
and unbatched runs alternate, in one process; every run builds fresh samplers and times warmup + sampling after one untimed iteration.

    python tools/batch_probe.py [--iter 60] [--reps 2] [--out profiles/batch_probe.jsonl] [--latents parallel]
"""
import argparse
import copy
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def shapes(iters):
    from stan4bart_amd import GroupTerm, generate_friedman_data, make_sampler_args
    from stan4bart_amd.cases import ihdp_case
    d = generate_friedman_data(4096, ranef=True, causal=True)
    x = d["x"]
    xb = x[:, [0, 1, 2, 4, 5, 6, 7, 8, 9]]
    gauss = make_sampler_args(d["y"], xb, X=np.column_stack([x[:, 3], d["z"]]), groups=[GroupTerm(d["g1"], None, "g.1"), GroupTerm(d["g2"], None, "g.2")],
                              iter=iters, warmup=iters // 2, bart_args={"n.trees": 75})
    return {"ihdp_binary_T75": ihdp_case(T=75, warmup=iters // 2, iter=iters), "gauss_n4096_ranef_T75": gauss}


def run(lib, args, C, batched):
    from stan4bart_amd import RRng
    from stan4bart_amd.abi import Sampler, SweepGroup
    samplers = []
    for c in range(C):
        a = copy.copy(args)
        rng = RRng(1000 + c)
        a.seed = int(rng.sample_int(2147483647, 1)[0])
        samplers.append(Sampler(lib, "s4b_", a, rng.state))
    g = SweepGroup(lib, "s4b_", 0, C) if batched else None
    for s in samplers:
        s.run(1, True, 0)          # untimed: first-sweep set-up
        if g is not None:
            g.join(s)
    errors = []

    def go(s):
        try:
            s.run(args.warmup, True, 0)
            s.disengage_adaptation()
            s.run(args.iter - args.warmup, False, 0)
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    th = [threading.Thread(target=go, args=(s,)) for s in samplers]
    t0 = time.perf_counter()
    [t.start() for t in th]
    [t.join() for t in th]
    wall = time.perf_counter() - t0
    st = None
    for s in samplers:
        if g is not None:
            g.leave(s)
        s.free()
    if g is not None:
        st = g.stats()
        g.free()
    if errors:
        raise errors[0]
    return C * args.iter / wall, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iter", type=int, default=60)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--chains", default="1,2,4,8,16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="ihdp,gauss", help="comma-separated prefixes of the shapes to run")
    ap.add_argument("--batched-only", action="store_true", help="only the batched runs (a kernel trace of the batched launches)")
    ap.add_argument("--latents", choices=("exact", "parallel"), default="exact", help="probit latents of the binary shape (bart_args latents)")
    o = ap.parse_args()
    from stan4bart_amd._lib import load_library
    lib = load_library()
    out = open(o.out, "w") if o.out else None
    for name, args in shapes(o.iter).items():
        if not any(name.startswith(p) for p in o.shapes.split(",")):
            continue
        if args.is_binary:
            args.latents = o.latents
        for C in [int(c) for c in o.chains.split(",")]:
            rates = {False: [], True: []}
            stats = None
            for _ in range(o.reps):
                for batched in ((True,) if o.batched_only else (False, True)):
                    r, st = run(lib, args, C, batched)
                    rates[batched].append(r)
                    stats = st if batched else stats
            ub = max(rates[False]) if rates[False] else None
            rec = dict(shape=name, latents=args.latents, chains=C, iter=o.iter, unbatched_it_s=ub, batched_it_s=max(rates[True]),
                       speedup=max(rates[True]) / ub if ub else None, all_unbatched=rates[False], all_batched=rates[True], group_stats=stats)
            print(json.dumps(rec), flush=True)
            if out:
                out.write(json.dumps(rec) + "\n")
                out.flush()


if __name__ == "__main__":
    main()
