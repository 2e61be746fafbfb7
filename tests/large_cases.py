"""Seeded random configurations at the sizes where k_sweep fills the device (n = 5e4 ... 1.04e6: up to 255 pass workgroups exchange their
bin partials), BART block only.  Used by tools/fuzz_large.py (campaigns of hundreds of seeds outside the suite) and by
tests/test_gpu_large.py (eight of them in the driver-run suite)."""
import numpy as np


def large_case(seed, n=None, iters=None, deep=None, k_chi=None, trees=None, split_probs=False, weights=False):
    """`n`, `iters` (warm-up, total), `deep` (True: trees of tens of leaves from the prior, i.e. hand-overs to k_step), `k_chi` ((df, scale) of a
    modeled k) and `trees` override what the seed drew; everything else stays the seed's.  `split_probs`: cgm(split.probs = ) with weights drawn from a
    generator of their own (the seed's other draws stay what they are) — the persistent sweep then runs as k_sweep_sp / k_sweep_few_sp.  `weights`: observation weights from a generator of their own, a
    scale between 1e-3 and 1 and a few weights a thousand times smaller than the rest (k_sweep_w); not for binary responses, not together with split_probs."""
    from stan4bart_amd import GroupTerm, make_sampler_args
    g = np.random.default_rng(500000 + seed)
    n0 = int(g.choice([g.integers(50000, 200000), g.integers(200000, 700000), g.integers(700000, 1044000)]))
    n = n0 if n is None else int(n)
    p = int(g.integers(1, 9))
    cols = [(g.random(n) < 0.3).astype(np.float64) if g.random() < 0.25 else (g.normal(size=n) if g.random() < 0.5 else g.random(n)) for _ in range(p)]
    xb = np.column_stack(cols)
    x4 = g.random(n)
    f = 3.0 * np.sin(2.0 * xb[:, 0]) + (xb[:, -1] > np.median(xb[:, -1])) * 2.0 + 1.5 * x4
    binary = bool(g.random() < 0.15) and n < 150000              # (probit latents are serial: keep those cases small)
    yc = f + g.normal(size=n) * g.choice([0.1, 1.0, 3.0])
    y = (yc > np.median(yc)).astype(np.float64) if binary else yc * g.choice([1.0, 1e-3, 250.0])
    bart_args = {"n.trees": int(g.integers(1, 13)), "n.cuts": int(g.choice([1, 5, 100])), "k": float(g.choice([0.5, 2.0, 4.0]))}
    r = g.random()
    if deep is not None:
        r = 0.4 if deep else 0.9
    if r < 0.3:
        bart_args.update(base=0.99, power=0.5)
    elif r < 0.45:
        bart_args.update(base=0.99, power=0.3, k=0.3)             # trees of tens of leaves from the prior: hand-overs
    if g.random() < 0.2:
        bart_args["useQuantiles"] = True
    warmup = int(g.integers(1, 5)); it = warmup + int(g.integers(2, 8))
    if iters is not None:
        warmup, it = iters
    if trees is not None:
        bart_args["n.trees"] = int(trees)
    if k_chi is not None:
        bart_args["k"] = ("chi", float(k_chi[0]), float(k_chi[1]))
    if split_probs:
        bart_args["split.probs"] = [float(w) for w in np.random.default_rng(900000 + seed).choice([0.05, 0.5, 1.0, 1.0, 3.0, 8.0], size=p)]
    groups = [GroupTerm(g.integers(1, 6, size=n), None, "g.1")] if g.random() < 0.4 else []
    w = None
    if weights and not binary and not split_probs:
        gw = np.random.default_rng(700000 + seed)
        # (weights of O(1) and below.  A weight multiplies an observation's precision; the reference — dbarts, restated in oracle/bart_ref.hpp — gives a branch with an
        # EMPTY leaf the log-likelihood -1e7 and compares it with the FULL integrated likelihood of the other branch, within-leaf sum of squares included, while the
        # device code carries the terms that do not cancel between two non-empty branches only: once sum of w d^2 / sigma^2 of a branch exceeds 2e7 — weights of 40 at
        # n = 4e5 — the reference ACCEPTS a rule that leaves a leaf empty and the device code rejects it: seed 79 of the first version of this generator)
        w = gw.uniform(0.25, 4.0, n) * float(gw.choice([1e-3, 0.03, 0.125, 1.0, 1.0]))
        w[gw.integers(0, n, 100)] *= 1e-3
    args = make_sampler_args(y, xb, X=x4[:, None], groups=groups, family="binomial" if binary else "gaussian", iter=it, warmup=warmup, bart_args=bart_args, weights=w,
                             x_test=xb[:50].copy() if g.random() < 0.3 else None)
    if bart_args.get("power") == 0.3:
        args.node_capacity = 1024
    return args, dict(n=n, p=p, binary=binary, **{k: v for k, v in bart_args.items() if k != "split.probs"}, split_probs=bool(split_probs), weights=w is not None)


def sized_case(n, seed=0, p=10, trees=8, iters=(2, 8), deep=False, weights=False, k_chi=None, split_probs=False, binary=False, joint=False, **kw):
    """Sampler arguments at the sizes that pick the fused (k_step) and the two-kernel (k_tree + k_control) tree updates (tests/test_gpu_sizes.py).
    numpy's generator (generate_friedman_data's R-compatible stream would take minutes at n = 1e7), p uniform covariates with n.cuts = 100: at these
    sizes every cut of an ordinary tree leaves thousands of observations on both sides, so no proposal can empty a leaf (the reference's empty-leaf
    rule, DESIGN.md 7, stays out of reach).  BART block only unless `joint` (then a fixed effect and a random intercept of 5 groups: the Stan block's O(N) sums).
    `deep`: base 0.99, power 0.3, k 0.3 and 1024 node slots (trees of tens of leaves: more than 8 bins per proposal, more than 64 node slots).
    `weights`: observation weights of O(1).  `k_chi`: (df, scale) of a modeled k.  `split_probs`: cgm(split.probs = ).  `binary`: probit latents (needs `joint`: a probit model of BART alone is refused as improper).  Other keywords go to make_sampler_args."""
    from stan4bart_amd import GroupTerm, make_sampler_args
    g = np.random.default_rng(800000 + seed)
    xb = np.empty((n, p), order="F")
    for j in range(p):
        xb[:, j] = g.random(n)
    f = 10.0 * np.sin(np.pi * xb[:, 0] * xb[:, 1]) + 20.0 * (xb[:, 2] - 0.5) ** 2 + 10.0 * xb[:, 3] + 5.0 * xb[:, 4]
    y = f + g.standard_normal(n)
    X, groups = None, []
    if joint:
        X = g.random(n)[:, None]
        y = y + 2.0 * X[:, 0]
        groups = [GroupTerm(g.integers(1, 6, size=n), None, "g.1")]
    if binary:
        y = (y > np.median(y)).astype(np.float64)
    bart_args = {"n.trees": int(trees), "n.cuts": 100}
    if deep:
        bart_args.update(base=0.99, power=0.3, k=0.3)
    if k_chi is not None:
        bart_args["k"] = ("chi", float(k_chi[0]), float(k_chi[1]))
    if split_probs:
        bart_args["split.probs"] = [float(v) for v in g.choice([0.05, 0.5, 1.0, 3.0, 8.0], size=p)]
    w = g.uniform(0.25, 4.0, n) if weights else None
    args = make_sampler_args(y, xb, X=X, groups=groups, family="binomial" if binary else "gaussian", iter=iters[1], warmup=iters[0],
                             bart_args=bart_args, weights=w, **kw)
    if deep:
        args.node_capacity = 1024
    return args


def stan_shape_case(n, K, terms, seed, hmc_mode, weights=False, ragged=False, iters=(6, 9), trees=4, max_treedepth=None, plain_init=False):
    """Sampler arguments whose PARAMETRIC model has a chosen shape (tests/test_gpu_stan_shapes.py and its CPU twin tests/test_stan_shapes.py): K
    fixed-effect columns, and one `(1 + slopes | g)` term per entry `(levels, n_slopes)` of `terms`, so q = sum levels * (1 + n_slopes) columns of Z
    and sum (1 + n_slopes) non-zeros per row.  These decide which of the Stan block's O(N) kernels runs, which instantiation and which branch in it.
    Standard-normal X and slopes, every level of every term occupied (level of row i: a seeded permutation of i mod levels), uniform BART covariates
    with n.cuts = 100 and a handful of trees: the tree side is not the subject (no proposal can empty a leaf).
    `weights`: observation weights of O(1).  `ragged`: a third of the LAST slope column is set to exactly 0 and those entries are left out of the CSR
    triplet (w, v, u) handed to create: the same matrix with fewer stored entries and a number of non-zeros that varies from row to row.
    `iters`: (warm-up, total).  `max_treedepth`: caps the trajectories where the oracle's O(N q) leapfrogs would take minutes.
    `plain_init`: the starting values (bart_offset_init, sigma_init) come from the least-squares fit on X alone instead of X and the level dummies
    of every grouping factor: for thousands of levels that fit costs ~10 s per case, and with more dummies than observations it is saturated
    (sigma_init = 1e-13).  Where a chain starts is not the subject here."""
    import stan4bart_amd.fit as fit
    from stan4bart_amd import GroupTerm
    g = np.random.default_rng(600000 + seed)
    p = 5
    xb = np.empty((n, p), order="F")
    for j in range(p):
        xb[:, j] = g.random(n)
    X = g.standard_normal((n, K)) if K else None
    y = 10.0 * np.sin(np.pi * xb[:, 0] * xb[:, 1]) + 10.0 * xb[:, 3] + g.standard_normal(n)
    if K:
        y = y + X @ g.uniform(-1.0, 1.0, K)
    groups, ragged_done = [], False
    for t, (levels, n_slopes) in enumerate(terms):
        assert 1 <= levels <= n, "every level must be occupied"
        lev = (g.permutation(n) % levels) + 1
        slopes = g.standard_normal((n, n_slopes)) if n_slopes else None
        if ragged and n_slopes and t == max(i for i, (_, s) in enumerate(terms) if s):
            slopes[g.random(n) < 1.0 / 3.0, n_slopes - 1] = 0.0
            ragged_done = True
        y = y + g.standard_normal(levels)[lev - 1] * 0.7
        for c in range(n_slopes):
            y = y + g.standard_normal(levels)[lev - 1] * 0.5 * slopes[:, c]
        groups.append(GroupTerm(lev, slopes, "g.%d" % (t + 1)))
    assert ragged_done or not ragged, "ragged needs a term with a slope"
    w = g.uniform(0.25, 4.0, n) if weights else None
    stan_args = {"hmc_mode": int(hmc_mode)}
    full_init = fit.init_fit
    if plain_init:
        fit.init_fit = lambda y_, Xc_, groups_, n_, binary_: full_init(y_, Xc_, [], n_, binary_)
    try:
        args = fit.make_sampler_args(y, xb, X=X, groups=groups, iter=iters[1], warmup=iters[0], bart_args={"n.trees": int(trees), "n.cuts": 100},
                                     weights=w, stan_args=stan_args)
    finally:
        fit.init_fit = full_init
    if max_treedepth is not None:
        args.max_treedepth = int(max_treedepth)
    if ragged:
        # (make_z_csr stores every coefficient of every row: drop the explicit zeros here)
        z = int(sum(args.p))
        keep = np.asarray(args.w).reshape(n, z) != 0.0
        assert not keep.all() and keep.any(axis=1).all()
        args.u = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
        args.w = np.asarray(args.w).reshape(n, z)[keep].copy()
        args.v = np.asarray(args.v).reshape(n, z)[keep].copy()
    return args


def stan_shape_of(args):
    """(K, q, non-zeros per row of Z: an int when every row stores the same number, else the tuple (min, max))."""
    K = 0 if args.X is None else np.asarray(args.X).reshape(len(args.y), -1).shape[1]
    q = int(sum(int(pi) * int(li) for pi, li in zip(args.p, args.l)))
    d = np.diff(np.asarray(args.u, dtype=np.int64)) if q else np.zeros(1, np.int64)
    return K, q, (int(d[0]) if d.min() == d.max() else (int(d.min()), int(d.max())))


# ---- the shapes of tests/test_gpu_stan_shapes.py (GPU against the oracle) and tests/test_stan_shapes.py (emulation against the oracle: identical data) --------
# name -> keywords of stan_shape_case (without hmc_mode).  Small q: cheap for the oracle, so these also run teacher-forced through ~45 iterations.
STAN_SMALL_SHAPES = {
    # k_stan_fused<8, *> (K = 5 .. 8) and <16, *> (K = 9 .. 16): first and last K of each, one random intercept
    "K5": dict(n=300, K=5, terms=[(4, 0)]),
    "K8": dict(n=300, K=8, terms=[(4, 0)]),
    "K8-weighted": dict(n=300, K=8, terms=[(4, 0)], weights=True),
    "K9": dict(n=300, K=9, terms=[(4, 0)]),
    "K16": dict(n=400, K=16, terms=[(4, 0)]),
    "K16-weighted": dict(n=400, K=16, terms=[(4, 0)], weights=True),
    # K + q = 64: beta, b travel in the kernel arguments (S_PAR_INLINE); 65: they are read from s.params
    "K12-q52": dict(n=500, K=12, terms=[(52, 0)]),
    "K12-q53-weighted": dict(n=500, K=12, terms=[(53, 0)], weights=True),
    # K > 16: not fused, the plain-double pipeline is the primary path; k_xt_e's last group has (K - 3) % 4 = 2, 1, 0 (0: a full group of 4) columns
    "K17": dict(n=400, K=17, terms=[(4, 0)]),
    "K20-weighted": dict(n=400, K=20, terms=[(4, 0)], weights=True),
    "K23": dict(n=500, K=23, terms=[(4, 0)]),
    # rows of Z: 4 non-zeros (the last register slot of the fixed-row path), 5 and 7 (general CSR loop; a term with p = 3 also takes the host's taped gradient), ragged
    "nz4-K8": dict(n=300, K=8, terms=[(5, 1), (3, 1)]),
    "nz5-K2": dict(n=400, K=2, terms=[(6, 2), (4, 1)]),
    "nz7-K9": dict(n=400, K=9, terms=[(5, 2), (4, 1), (3, 1)]),
    "ragged-K5": dict(n=400, K=5, terms=[(5, 1), (3, 1)], ragged=True),
    # no X column at all, a sloped term
    "K0-sloped": dict(n=300, K=0, terms=[(6, 1)]),
}
# Large q: free-running and short (the oracle's leapfrogs cost O(q) and more), intercept-only terms.
STAN_LARGE_SHAPES = {
    # q = 512: the last q with one LDS histogram per wave; n < 256 (one partly filled workgroup), so three terms are needed to occupy every level: 3 non-zeros per row
    "q512-n250": dict(n=250, K=2, terms=[(250, 0), (250, 0), (12, 0)], iters=(6, 9), plain_init=True),
    # q = 513: the first q with one histogram shared by the four waves; <8>
    "q513-K5": dict(n=3000, K=5, terms=[(513, 0)], iters=(6, 9)),
    # q = 2100: fusedLds_ passes 48 KiB (hipFuncSetAttribute opt-in); M = 2103 > 2048: the host's hash-map Gram.  n = 700 000 > 2048 * 256 = 524 288:
    # the grid-stride loop and the two-deep prefetch of k_stan_fused run twice on a third of the threads
    "q2100-n700k": dict(n=700_000, K=3, terms=[(2100, 0)], iters=(4, 6), max_treedepth=6, plain_init=True),
    # q = 4096 = S_QMAX, K = 9: <16> with the largest LDS request there is (64 KiB histogram + 32 KiB of b)
    "q4096-K9": dict(n=9000, K=9, terms=[(4096, 0)], iters=(3, 4), max_treedepth=5, plain_init=True),
    # q = 4097: not fused; k_zt_chunks with 4097 columns
    "q4097": dict(n=9000, K=2, terms=[(4097, 0)], iters=(3, 4), max_treedepth=5, plain_init=True),
}


def stan_kernel_branch(K, q, nz):
    """Which O(N) kernel of the Stan block a parametric model of this shape runs, which instantiation and which branches inside it: a function of
    (K, q, row lengths of Z) alone, restated here from stan4bart_amd/csrc/dev_hip.hip (creation of the device arrays, launch_stan_fused, k_stan_fused)
    with the constants READ from that file, so that a moved threshold changes what the tests expect of their cases instead of quietly moving the
    cases to another kernel.  `nz`: stan_shape_of(args)[2].  Returns a dict: fused (False: k_stan_inputs + k_xt_e + k_zt_chunks + k_stan_finalize is the
    primary path), kmax, zfixed (-1: the CSR loop), ncopy (LDS histograms per workgroup), lds (dynamic bytes), par_inline, xt_e_launches, xt_e_last."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stan4bart_amd", "csrc", "dev_hip.hip")).read()

    def const(name):
        return int(re.search(r"constexpr int " + name + r" = (\d+);", src).group(1))
    sblock, qmax, zmax, inline = const("SBLOCK"), const("S_QMAX"), const("S_ZMAX"), const("S_PAR_INLINE")
    assert "stanFused_ = K_ <= 16 && q_ <= S_QMAX;" in src and "(size_t)q * 16 * (SBLOCK / 64) <= 32768 ? SBLOCK / 64 : 1" in src
    assert "for (int k0 = 3; k0 < K_; k0 += 4)" in src
    fused = K <= 16 and q <= qmax
    waves = sblock // 64
    ncopy = waves if q * 16 * waves <= 32768 else 1
    xt = len(range(3, K, 4))
    return dict(fused=fused, kmax=2 if K <= 2 else 4 if K <= 4 else 8 if K <= 8 else 16,
                zfixed=nz if isinstance(nz, int) and 0 <= nz <= zmax and q else -1, ncopy=ncopy,
                lds=q * 16 * ncopy + (K + q) * 8 + 16, par_inline=K + q <= inline, xt_e_launches=xt, xt_e_last=(K - 3) - 4 * (xt - 1) if xt else 0)
