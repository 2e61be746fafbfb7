"""s4b_partial_dependence on the device (stan4bart_amd/csrc/dev_pd.inc: k_partial_dependence<staged>, k_partial_dependence<global>, k_summary_fold)
against predict_bart of the overwritten rows per grid point (tests/pd_cases.py: the model, the derived bound, the tree-order restatement).  Shapes are
stated in the kernel's own constants, read from the `info` words of a call or from the source: rows around one tile and into a workgroup's second
tile; 1, 63 and 64 grid points (65 refused); 1, 2 and an odd number of draws (the staging buffers' parity); affected-tree counts 0, 1, 3, 4, 5 and
all, around the four trees walked at once, asserted from get_kept_trees(); the largest draw below, at and one node beyond the staging buffer; a joint
grid of two predictors; grid values on, next to and far from a cut value; the linear parts, both links, a binary response, weights; per-draw
response scales; determinism; refusals before any launch; the whole Python interface.

The chains are tiny (n = 400, T <= 25, a dozen iterations); a reference is computed once per case and shared by the routes."""
import os
import re

import numpy as np
import pytest

import pd_cases as pc
import readout_cases as rc
import summary_cases as sc
from conftest import make_sampler

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALK = 4          # PS_WALK: trees walked at once per thread (asserted from the source in _constants)


def _report(line):
    print(line)


def _constants():
    src = open(os.path.join(ROOT, "stan4bart_amd", "csrc", "dev_summary.inc")).read()
    pd = open(os.path.join(ROOT, "stan4bart_amd", "csrc", "dev_pd.inc")).read()
    c = dict(tile=int(re.search(r"constexpr int PS_BLOCK = (\d+);", src).group(1)), walk=int(re.search(r"constexpr int PS_WALK = (\d+);", src).group(1)),
             cap=int(re.search(r"constexpr int PS_STAGE_NODES = (\d+);", src).group(1)), grid_max=int(re.search(r"constexpr int PD_GRID_MAX = (\d+);", pd).group(1)))
    assert c["walk"] == WALK
    return c


@pytest.fixture(scope="module")
def gauss(hip_lib):
    c = pc.Chain(hip_lib, "s4b_", rc._friedman(n=400, T=25, warmup=4, iter=17, ranef=False))
    yield c
    c.close()


@pytest.fixture(scope="module")
def binary(hip_lib):
    c = pc.Chain(hip_lib, "s4b_", rc._binary(n=400, T=11, warmup=6, iter=19), rows=1300)
    yield c
    c.close()


def _grid(chain, v, G, seed=0):
    """G values over the training range of predictor v widened by a fifth, in no order."""
    col = np.asarray(chain.args.x_bart)[:, v]
    lo, hi = col.min(), col.max()
    return np.random.default_rng(900 + seed).uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), G)


def _busiest(chain, S):
    """The predictor with the most affected trees in the sampler of S draws."""
    return int(np.argmax([chain.hit(S, v).sum() for v in range(chain.P)]))


_REF = {}


def _case(chain, S, rows, vars, grid, what, link=0, M=0, E=0, weights=False, offset=False, seed=0, **kw):
    """One call on the stored sampler with S draws over the first `rows` rows against the model; the reference of a case is computed once."""
    smp, x = chain.stored[S], np.asfortranarray(chain.x[:rows])
    parts = sc.linear_parts(rows, S, M, E, seed=seed)
    w = sc.weight_vectors(rows, 3, seed=seed)[2] if weights else None          # zeros and negative entries
    off = 1e3 * float(chain.range[1] - chain.range[0]) * np.random.default_rng(seed).uniform(-1.0, 1.0, rows) if offset else None
    got = smp.partial_dependence(x, vars, grid, offset=off, link=link, weights=w, **parts, **kw)
    hit = chain.hit(S, vars)
    assert got["draws"] == S and got["info"]["launches"] == 2
    assert got["info"]["largest_affected"] == hit.sum(axis=1).max() and got["info"]["total_affected"] == hit.sum(), (what, got["info"])
    key = (id(chain), S, rows, tuple(np.atleast_1d(vars)), np.asarray(grid).tobytes(), link, M, E, weights, offset, seed)
    if key not in _REF:
        _REF[key] = chain.reference(S, rows, vars, grid, weights=w, link=link, offset=off, **parts)
    pc.assert_pd(got, *_REF[key], what, _report)
    return got, dict(x=x, offset=off, link=link, weights=w, **parts)


def test_rows_around_a_tile_and_a_second_tile(gauss):
    k = _constants()
    tile = k["tile"]
    assert gauss.stored[5].partial_dependence(gauss.x[:1], 0, [0.5])["info"]["rows_per_tile"] == tile and len(gauss.x) >= 2 * tile + 1
    v = _busiest(gauss, 5)
    grid = _grid(gauss, v, 5)
    for rows, kw in ((1, {}), (tile - 1, {}), (tile, {}), (tile + 1, {}), (2 * tile + 1, dict(max_workgroups=2))):
        res = {}
        for route in ("staged", "global"):
            res[route], _ = _case(gauss, 5, rows, v, grid, f"rows {rows} {route}", M=1, E=1, weights=True, route=route, **kw)
            want = min(-(-rows // tile), kw.get("max_workgroups", 1 << 30))
            assert res[route]["info"]["workgroups"] == want and res[route]["info"]["route"] == (1 if route == "staged" else 2)
        assert np.array_equal(res["staged"]["pd"], res["global"]["pd"]), f"rows {rows}: the two routes differ"
    # 2 workgroups x tile + 1 rows: workgroup 0 comes round to a second tile, where its partials accumulate
    assert res["global"]["info"]["workgroups"] == 2 and 2 * tile < rows


@pytest.mark.parametrize("G", [1, 63, 64])
def test_grid_sizes(gauss, G):
    k = _constants()
    assert k["grid_max"] == 64
    v = _busiest(gauss, 2)
    for route in ("staged", "global"):
        got, _ = _case(gauss, 2, 70, v, _grid(gauss, v, G, seed=G), f"G {G} {route}", M=1, route=route)
        assert got["pd"].shape == (2, G)
    if G == 64:
        with pytest.raises(RuntimeError, match="between 1 and 64 grid points per call, not 65"):
            gauss.stored[2].partial_dependence(gauss.x[:70], v, _grid(gauss, v, 65))
        assert gauss.stored[2].pd_info["launches"] == 0


@pytest.mark.parametrize("S", [1, 2, 5])
def test_draws_one_two_and_odd(gauss, S):
    tile = _constants()["tile"]
    v = _busiest(gauss, S)
    res = {}
    for route in ("staged", "global"):
        res[route], _ = _case(gauss, S, tile + 37, v, _grid(gauss, v, 6), f"S {S} {route}", M=2, E=2, route=route)
    assert np.array_equal(res["staged"]["pd"], res["global"]["pd"])


def test_affected_counts_around_the_walk_width(gauss, binary):
    """0, 1, 3, 4, 5 affected trees in a draw (four trees are walked at once), T = 11 and 25: neither a multiple of four."""
    assert binary.T % WALK and gauss.T % WALK
    seen = set()
    for chain, S in ((binary, 13), (gauss, 1)):
        for v in range(chain.P):
            counts = set(chain.hit(S, v).sum(axis=1).tolist())
            if counts & ({0, 1, 3, 4, 5} - seen) or v == 0:
                res = {}
                for route in ("staged", "global"):
                    res[route], _ = _case(chain, S, 200, v, _grid(chain, v, 3, seed=v), f"{'binary' if chain is binary else 'gauss'} predictor {v}, "
                                          f"affected per draw {sorted(counts)}, {route}", route=route)
                assert np.array_equal(res["staged"]["pd"], res["global"]["pd"])
                seen |= counts
    assert {0, 1, 3, 4, 5} <= seen, f"affected-tree counts covered: {sorted(seen)}"


def test_predictor_no_tree_uses(hip_lib):
    """A predictor that is constant in training carries no rule: every tree is walked once, no tree per grid point, and the result is bit-equal across
    the grid.  As the second predictor of a pair it must change nothing."""
    args = rc._friedman(n=400, T=25, warmup=4, iter=9, ranef=False)
    xb = np.array(args.x_bart, order="F")
    xb[:, 6] = 0.5
    args.x_bart = xb
    chain = pc.Chain(hip_lib, "s4b_", args, steps=(2, 3), rows=300)
    try:
        assert not chain.hit(5, 6).any()
        grid = np.r_[-np.inf, 0.1, 0.5, 0.9, np.inf]
        for route in ("staged", "global"):
            got, _ = _case(chain, 5, 300, 6, grid, f"unused predictor {route}", M=1, route=route)
            assert got["info"]["largest_affected"] == 0 and got["info"]["total_affected"] == 0
            assert np.array_equal(got["pd"], np.repeat(got["pd"][:, :1], len(grid), axis=1)), "no tree moves, but the grid points differ"
        v = _busiest(chain, 5)
        one = _grid(chain, v, 7)
        pair = np.column_stack([one, np.linspace(-1.0, 2.0, 7)])
        a, _ = _case(chain, 5, 300, v, one, "one predictor")
        for vs, gr in (([v, 6], pair), ([6, v], pair[:, ::-1])):
            b, _ = _case(chain, 5, 300, vs, gr, f"pair {vs}, the other predictor in no tree")
            assert np.array_equal(a["pd"], b["pd"]) and b["info"]["total_affected"] == a["info"]["total_affected"]
    finally:
        chain.close()


def test_one_predictor_in_total(hip_lib):
    """P = 1: every tree with a rule is affected — the walk-once group holds only the trees that are a single leaf."""
    args = rc._friedman(n=400, T=7, warmup=4, iter=9, ranef=False)
    args.x_bart = np.asfortranarray(np.array(args.x_bart)[:, :1])
    chain = pc.Chain(hip_lib, "s4b_", args, steps=(2, 3), rows=300)
    try:
        hit = chain.hit(5, 0)
        stumps = np.array([[np.sum((chain.trees[5]["sample"] == k) & (chain.trees[5]["tree"] == t)) == 1 for t in range(7)] for k in range(5)])
        assert np.array_equal(hit, ~stumps) and (hit.sum(axis=1) == 7).any(), "no draw has every tree affected (an empty walk-once group)"
        for route in ("staged", "global"):
            _case(chain, 5, 300, 0, _grid(chain, 0, 9), f"P = 1 {route}", route=route)
    finally:
        chain.close()


def test_routes_around_the_staging_buffer(gauss):
    S, T, cap = gauss.draws, gauss.T, _constants()["cap"]
    v = _busiest(gauss, S)
    grid = _grid(gauss, v, 4)
    auto, inp = _case(gauss, S, 1100, v, grid, "automatic route")
    x = inp["x"]
    largest = auto["info"]["largest_draw_nodes"]
    assert largest >= np.bincount(gauss.trees[S]["sample"]).max()          # (node slots of the draw: at least its entries)
    assert largest + 1 <= cap and auto["info"]["route"] == 1
    assert auto["info"]["staging_bytes"] == 16 * (-(-largest // 64) * 64) + 8 * T
    seen = set()
    for knob in (largest + 1, largest, largest - 1):          # the largest draw below the buffer, filling it exactly, one node beyond it
        got = gauss.stored[S].partial_dependence(x, v, grid, stage_nodes=knob)
        want = 1 if largest <= knob else 2
        assert got["info"]["route"] == want and got["info"]["staging_bytes"] == (16 * knob + 8 * T if want == 1 else 0), (knob, got["info"])
        assert np.array_equal(got["pd"], auto["pd"]), f"stage_nodes {knob}: the two routes differ"
        seen.add(want)
    assert seen == {1, 2}
    forced = gauss.stored[S].partial_dependence(x, v, grid, route="global")
    assert forced["info"]["route"] == 2 and np.array_equal(forced["pd"], auto["pd"])
    live = gauss.live.partial_dependence(x, v, grid)          # the live sampler holds the same kept trees
    assert np.array_equal(live["pd"], auto["pd"]) and live["info"] == auto["info"]


def test_two_predictors_on_a_joint_grid(gauss):
    S = 5
    order = np.argsort([gauss.hit(S, v).sum() for v in range(gauss.P)])
    v0, v1 = int(order[-1]), int(order[-2])
    a, b = _grid(gauss, v0, 4, seed=1), _grid(gauss, v1, 3, seed=2)
    pair = np.column_stack([np.repeat(a, 3), np.tile(b, 4)])
    both = gauss.hit(S, [v0, v1]).sum(axis=1)
    assert (both > gauss.hit(S, v0).sum(axis=1)).any(), "the second predictor affects no further tree"
    res = {}
    for route in ("staged", "global"):
        res[route], _ = _case(gauss, S, 700, [v0, v1], pair, f"pair ({v0}, {v1}) {route}", M=1, E=1, route=route)
    assert np.array_equal(res["staged"]["pd"], res["global"]["pd"])
    swapped, _ = _case(gauss, S, 700, [v1, v0], pair[:, ::-1], f"pair ({v1}, {v0})", M=1, E=1)
    assert np.array_equal(swapped["pd"], res["staged"]["pd"])          # the same trees in the same order, the same bins


def test_grid_values_at_and_around_a_cut(gauss):
    S = gauss.draws
    trees = gauss.trees[S]
    last = {k: a[trees["sample"] == S - 1] for k, a in trees.items()}
    (rv, rcut), _ = rc.rule_list(last, 0)
    assert len(rv), "the last draw has no root rule"
    v, cut = int(rv[0]), float(rcut[0])
    col = np.asarray(gauss.args.x_bart)[:, v]
    far = 10.0 * (col.max() - col.min()) + 1.0
    grid = np.array([cut, np.nextafter(cut, np.inf), np.nextafter(cut, -np.inf), np.inf, -np.inf, col.max() + far, col.min() - far, 1e300, -1e300])
    for route in ("staged", "global"):
        got, _ = _case(gauss, S, 500, v, grid, f"cut value of predictor {v} {route}", route=route)
        pd = got["pd"]
        assert np.array_equal(pd[:, 0], pd[:, 2]), "the cut value itself and the double below it must both go left"
        assert pd[S - 1, 0] != pd[S - 1, 1], "the double above a root rule's cut value goes right: the draw's average must move"
        assert np.array_equal(pd[:, 3], pd[:, 5]) and np.array_equal(pd[:, 3], pd[:, 7]) and np.array_equal(pd[:, 4], pd[:, 6]) and np.array_equal(pd[:, 4], pd[:, 8])
        assert not np.array_equal(pd[:, 3], pd[:, 4])


@pytest.mark.parametrize("M,E", [(0, 0), (17, 0), (0, 1), (17, 3)])
def test_linear_parts(gauss, M, E):
    rows = _constants()["tile"] + 5
    v = _busiest(gauss, 5)
    for offset, weights in ((False, False), (True, True)):
        _, inp = _case(gauss, 5, rows, v, _grid(gauss, v, 4), f"M {M} E {E} offset {offset} weights {weights}", M=M, E=E, offset=offset, weights=weights, seed=M + E)
    if E > 1:
        ix = inp["ell_index"]
        assert (ix == -1).any() and len({int(n) for n in (ix >= 0).sum(axis=1)}) > 1, "the padding is not ragged"
    if weights:
        assert (inp["weights"] == 0).any() and (inp["weights"] < 0).any()


def test_links_and_binary_response(gauss, binary):
    assert binary.binary and not gauss.binary
    for chain, name in ((binary, "binary"), (gauss, "gauss")):
        v = _busiest(chain, 5)
        for link in (1, 0):
            for weights in (False, True):
                got, _ = _case(chain, 5, 400, v, _grid(chain, v, 5), f"{name} link {link} weights {weights}", link=link, M=2, E=1, weights=weights, seed=link)
            if link and not weights:
                assert np.all((got["pd"] >= 0) & (got["pd"] <= 1))


def test_per_draw_response_scales(hip_lib):
    """Warm-up (the scale moves) and sampling runs interleaved on one sampler, as readout_cases.check_per_draw_scale builds one: every draw under its own scale."""
    args = rc._friedman(n=400, T=12, warmup=12, iter=20, ranef=False)
    s = make_sampler(hip_lib, "s4b_", args)
    try:
        ranges = []
        for _ in range(4):
            s.run(3, True)
            s.run(2, False)
            ranges += [s.get_bart_data_range()] * 2
        ranges = np.array(ranges)
        assert len(np.unique(ranges[:, 1] - ranges[:, 0])) >= 3, "the kept draws do not carry distinct response scales"
        trees = s.get_kept_trees()
        x = np.asfortranarray(rc.new_rows(args.x_bart, 300, seed=5))
        v = int(np.argmax([pc.affected(trees, u, 8, 12).sum() for u in range(x.shape[1])]))
        col = np.asarray(args.x_bart)[:, v]
        grid = np.linspace(col.min(), col.max(), 5)
        ref, bound = pc.reference(s.predict_bart, trees, ranges, False, x, v, grid)
        for route in ("staged", "global"):
            got = s.partial_dependence(x, v, grid, route=route)
            assert got["draws"] == 8
            pc.assert_pd(got, ref, bound, f"per-draw scale {route}", _report)
    finally:
        s.free()


def test_same_call_twice_and_live_and_stored_are_bit_identical(gauss):
    rows = 2 * _constants()["tile"] + 1
    v = _busiest(gauss, 13)
    grid = _grid(gauss, v, 7)
    for route in ("staged", "global"):
        a, inp = _case(gauss, 13, rows, v, grid, f"determinism {route}", link=1, M=3, E=3, offset=True, weights=True, route=route, max_workgroups=2)
        x = inp.pop("x")
        b = gauss.stored[13].partial_dependence(x, v, grid, route=route, max_workgroups=2, **inp)
        c = gauss.live.partial_dependence(x, v, grid, route=route, max_workgroups=2, **inp)
        assert np.array_equal(a["pd"], b["pd"]), route
        assert np.array_equal(a["pd"], c["pd"]) and c["info"] == a["info"], route


def test_refusals_come_before_any_launch(hip_lib, gauss):
    rows, S = 50, 13
    x = np.asfortranarray(gauss.x[:rows])
    live = gauss.live

    def refused(match, vars=0, grid=(0.25, 0.5), samplers=None, **kw):
        before = live.get_counters()
        for smp in samplers or (live, gauss.stored[S]):
            with pytest.raises(RuntimeError, match=match):
                smp.partial_dependence(x, vars, np.asarray(grid, dtype=np.float64), **kw)
            assert smp.pd_info["launches"] == 0 and smp.pd_info["route"] == 0 and not any(smp.pd_info.values())
        assert np.array_equal(live.get_counters(), before), "a refused call launched something"
    refused(r"predictor 9 outside \[0, 9\)", vars=gauss.P)
    refused(r"predictor -1 outside", vars=-1)
    refused(r"predictor 9 outside", vars=[0, gauss.P], grid=[[0.1, 0.2]])
    refused("the two varied predictors must differ", vars=[3, 3], grid=[[0.1, 0.2]])
    refused("the grid holds a NaN", grid=[0.1, np.nan])
    refused("grid points per call, not 0", grid=np.zeros(0))
    refused("grid points per call, not 65", grid=np.linspace(0, 1, 65))
    refused("between 0 and 1 weight vectors, not 2", weights=np.ones((2, rows)))
    refused("link must be 0", link=2)
    fresh = make_sampler(hip_lib, "s4b_", gauss.args)          # keep_trees, but no sampling run yet
    try:
        refused("holds no kept draws", samplers=(fresh,))
    finally:
        fresh.free()
    before = live.get_counters()
    ok = live.partial_dependence(x, 0, [0.25, 0.5])
    assert ok["info"]["launches"] == 2 and live.get_counters()[2] == before[2] + 2


def test_whole_interface(hip_lib):
    """Stan4bartFit.partial_dependence on a two-chain fit with fixed effects and a random slope term (unseen levels among the new rows) against the loop
    over fit.predict with the column replaced, then the row mean; a 70-point grid split into two calls and joined; the default grid."""
    from stan4bart_amd import GroupTerm, generate_friedman_data
    from stan4bart_amd.abi import Sampler
    from stan4bart_amd.generics import PD_LEVQUANTS, stan4bart
    d = generate_friedman_data(120, ranef=True, causal=True, p=10)
    x = d["x"]
    xb, X = x[:, [j for j in range(10) if j != 3]], np.column_stack([x[:, 3], d["z"]])
    groups = [GroupTerm(d["g1"], x[:, 3], "g.1"), GroupTerm(d["g2"], None, "g.2")]
    fit = stan4bart(d["y"], xb, X=X, groups=groups, chains=2, seed=99, iter=14, warmup=6, bart_args={"n.trees": 9, "keepTrees": True},
                    make_sampler=lambda a, st: Sampler(hip_lib, "s4b_", a, st))
    try:
        m = 45
        g = np.random.default_rng(11)
        lev1 = np.asarray(d["g1"])[:m].copy()
        lev1[::4] = 6 + (np.arange(len(lev1[::4])) % 2)          # g.1 has five levels: 6 and 7 are unseen
        new = [GroupTerm(lev1, x[:m, 3] + 0.25, "g.1"), GroupTerm(np.asarray(d["g2"])[:m], None, "g.2")]
        xb_new, X_new, off = rc.new_rows(xb, m, seed=4), X[:m] + g.normal(size=(m, 2)), g.normal(size=m)
        trees = [s.get_kept_trees() for s in fit.samplers]
        v = int(np.argmax([pc.affected(trees[0], u, 8, 9).sum() for u in range(9)]))
        grid = np.linspace(xb[:, v].min(), xb[:, v].max(), 4)
        got = fit.partial_dependence(v, xb_new, grid=grid, X=X_new, groups=new, offset=off, seed=7, combine_chains=False)
        assert got["pd"].shape == (4, 8, 2) and np.array_equal(got["grid"], grid)
        ix, val, coef = fit._ell_random(new, True, np.random.default_rng(7))
        assert ix.max() >= fit.stan[fit._rows("b.")].shape[0], "no unseen level reached the table"
        beta = fit.stan[fit._rows("beta.")]
        loop = np.stack([fit.predict(x_bart=pc.overwritten(xb_new, v, c), X=X_new, groups=new, offset=off, combine_chains=False, seed=7).astype(np.longdouble)
                        .mean(axis=0) for c in grid])          # [G, iter, chain]
        worst = 0.0
        for c, smp in enumerate(fit.samplers):
            ref, bound = pc.reference(smp.predict_bart, trees[c], smp.get_bart_data_range(), False, xb_new, v, grid, offset=off, dense=X_new - fit.X_means,
                                      dense_coef=beta[:, :, c].T, ell_index=ix, ell_value=val, ell_coef=coef[c])
            r_model = rc.bound_ratio(got["pd"][:, :, c].T, ref, bound)
            # once for the device and once more for the double-precision arithmetic of fit.predict itself
            r_loop = rc.bound_ratio(got["pd"][:, :, c], loop[:, :, c].astype(np.float64), 2.0 * bound.T)
            print(f"whole interface, chain {c}: max |device - model| / bound = {r_model:.3g}, max |device - mean of fit.predict| / (2 x bound) = {r_loop:.3g}")
            worst = max(worst, r_model, r_loop)
        assert worst <= pc.BOUND_FACTOR, worst
        pooled = fit.partial_dependence(v, xb_new, grid=grid, X=X_new, groups=new, offset=off, seed=7)
        assert pooled["pd"].shape == (4, 16) and np.array_equal(pooled["pd"][:, :8], got["pd"][:, :, 0]) and np.array_equal(pooled["pd"][:, 8:], got["pd"][:, :, 1])
        np.testing.assert_allclose(pooled["mean"], pooled["pd"].mean(axis=1))
        assert np.all(pooled["lower"] <= pooled["mean"]) and np.all(pooled["mean"] <= pooled["upper"])
        # 70 grid points: two calls per chain (64 + 6), joined in the grid's order
        long = np.random.default_rng(3).uniform(xb[:, v].min(), xb[:, v].max(), 70)
        whole = fit.partial_dependence(v, xb_new, grid=long, type="indiv.bart")
        head, tail = fit.partial_dependence(v, xb_new, grid=long[:64], type="indiv.bart"), fit.partial_dependence(v, xb_new, grid=long[64:], type="indiv.bart")
        assert whole["pd"].shape == (70, 16) and np.array_equal(whole["pd"][:64], head["pd"]) and np.array_equal(whole["pd"][64:], tail["pd"])
        bart = np.stack([np.concatenate([s.predict_bart(pc.overwritten(xb_new, v, c)) for s in fit.samplers], axis=1).mean(axis=0) for c in long])
        assert len({tuple(r) for r in bart}) > 2 and not np.array_equal(bart[:6], bart[64:]), "the grid points do not tell the pieces' order apart"
        np.testing.assert_allclose(whole["pd"], bart, rtol=1e-12)          # every grid point at its own place
        # the default grid: the stated quantiles of the column; of a pair their product
        default = fit.partial_dependence(v, xb_new, type="indiv.bart")
        assert np.array_equal(default["grid"], np.quantile(xb_new[:, v], PD_LEVQUANTS)) and default["pd"].shape == (11, 16)
        pair = fit.partial_dependence((v, (v + 1) % 9), xb_new, type="indiv.bart")
        assert pair["grid"].shape == (121, 2) and pair["pd"].shape == (121, 16)
        assert np.array_equal(pair["grid"][:, 0], np.repeat(default["grid"], 11))
    finally:
        fit.close()
