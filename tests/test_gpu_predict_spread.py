"""s4b_predict_spread on the device (stan4bart_amd/csrc/readout_spread.inc: k_predict_values / k_contrast_values unchanged, k_spread_reduce,
k_spread_fold, k_spread_finish, k_level_rows and k_row_quantiles unchanged over the [(4 + 2 T) x S] matrix) against numpy in long double on the full
matrix (tests/spread_cases.py: the model, the bounds, the thresholds).  The smallest shapes at which the reduction can go wrong: 1, 127, 128, 129 and
1 100 rows, the last in 9 chunks of exactly one slab, in 3 and in 1 (the same bits); 1, 4 and 65 pooled draws (a second block of lanes with one live
lane, pooled from samplers of different lengths); T = 0 (no LDS), 1, 5 and 64 (65 KiB of dynamic LDS), -inf and +inf among finite thresholds, the
count of compares and the search for the bin (the same bits); no weights, random weights, a slab of zero weights, an indicator, dyadic weights; one
arm and two arms, identity and probit link; both routes, live and stored samplers; the weights times 2 and the swapped arms bit for bit;
predict_summary and predict_contrast as cross-checks of the mean; the refusals before any launch; the device bytes; the Python interface with
bayes_R2 against predict's matrix.

share_above at t = -inf is asserted to be exactly 1 without weights and with dyadic weights (every sum of them is exact in double, in any order); with
arbitrary weights the sum over the bins in slab order and the host's W in row order differ by roundings, and it is compared within its bound.

Small Friedman chains, as tests/test_gpu_predict_projection.py builds them (its Chain and its reference values are used as they are): n = 100, 5
trees, stored samplers of 1, 4, 9 and 64 draws; a binary chain (11 trees; 5 and 13 draws) for link 1.  Measured on an MI355X, the largest
|device - model| / bound of the module: min and max 0.49 (their bound is the value kernel's own), mean 0.16, part_above 0.14, share_above 0.023,
sd 1e-4; over the draws mean 0.12, m2 0.019, quantiles 0.21 (allowed: 4)."""
import ctypes as C
import struct

import numpy as np
import pytest

import group_cases as gc
import quantile_cases as qc
import readout_cases as rc
import spread_cases as sp
from test_gpu_predict_projection import Chain, _values

pytestmark = pytest.mark.gpu
WORST = {}
PROBS = (0.025, 0.5, 0.975, 0.0, 1.0, 1.0 / 3.0)
FLOATS = ("draws", "mean", "m2", "quantiles")


def _report(line):
    print(line)


def _note(ratios):
    for k, r in ratios.items():
        WORST[k] = max(WORST.get(k, 0.0), r)


@pytest.fixture(scope="module")
def gauss(hip_lib):
    c = Chain(hip_lib, rc._friedman(n=100, T=5, warmup=4, iter=4 + 64, ranef=False), rows=1100, steps=(1, 3, 5, 55))
    yield c
    c.close()
    print("predict_spread, largest |device - model| / bound of this module: " + ", ".join(f"{k} {r:.3g}" for k, r in WORST.items()))


@pytest.fixture(scope="module")
def binary(hip_lib):
    c = Chain(hip_lib, rc._binary(n=400, T=11, warmup=6, iter=19), rows=300, steps=(1, 1, 3, 8))
    yield c
    c.close()


def _case(chain, lens, rows, T, what, weights=None, probs=PROBS, values=None, infs=(False, False), thresholds=None, sampler=None, **call):
    """One pooled call through the C-ABI against the model.  The finite thresholds lie midway between adjacent reference values."""
    kw, x, bx = _values(chain, lens, rows, **(values or {}))
    th = sp.thresholds_for(x, T, *infs) if thresholds is None else np.asarray(thresholds, dtype=np.float64)
    ref, bd = sp.model(x, bx, weights, th, probs)
    got = (sampler or chain.stored[lens[0]]).predict_spread(thresholds=th, weights=weights, probs=probs, **kw, **call)
    S, info = sum(lens), got["info"]
    assert got["draws_pooled"] == S and info["draws"] == S and got["names"] == sp.names(len(th)), info
    _note(sp.assert_spread(got, ref, bd, what, _report, weighted=weights is not None))
    return got, (ref, bd), dict(kw, thresholds=th, weights=weights, probs=probs)


def _same_bits(a, b, what, keys=FLOATS + ("weight",)):
    for k in keys:
        assert (a.get(k) is None) == (b.get(k) is None), (what, k)
        if a.get(k) is not None:
            assert np.array_equal(a[k], b[k]), f"{what}: {k} differs"


# ---- slab edges and chunking -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 127, 128, 129, 1100])
def test_slab_edges_and_chunking(gauss, rows):
    S, T = 9, 5
    w = np.random.default_rng(rows).uniform(0.25, 2.0, rows)
    res = {}
    for name, Cr in (("C 128", 128), ("C 384", 384), ("one chunk", 0)):
        res[name], _, _ = _case(gauss, (S,), rows, T, f"{rows} rows, {name}", weights=w, values=dict(M=2, offset=True), infs=(True, True), scratch_bytes=Cr * 8 * S)
        info = res[name]["info"]
        want = min(rows, Cr) if Cr else rows
        assert info["rows_per_chunk"] == want and info["chunks"] == -(-rows // want) and info["launches"] == 3 * info["chunks"] + 3, info
    _same_bits(res["C 128"], res["C 384"], f"{rows} rows: C 128 and C 384")
    _same_bits(res["C 128"], res["one chunk"], f"{rows} rows: C 128 and one chunk")
    D = res["one chunk"]["draws"]
    assert np.all(D[4] <= 1.0 + 1e-12) and np.all(D[4 + T - 1] == 0.0) and np.all(D[4 + 2 * T - 1] == 0.0), "t = +inf: not exactly 0"
    if rows == 1:          # one row: its value, no spread
        assert np.array_equal(D[0], D[2]) and np.array_equal(D[2], D[3]) and np.all(D[1] == 0.0) and np.all(D[4] == 1.0)
        x1 = gauss.stored[S].predict_spread(**_values(gauss, (S,), 1, M=2, offset=True)[0], outputs=("draws",))["draws"]
        assert np.array_equal(x1[0], D[0]), "one row: the mean depends on the weight"
    if rows == 1100:
        assert [res[k]["info"]["chunks"] for k in ("C 128", "C 384", "one chunk")] == [9, 3, 1]
        # a scratch limit that is no multiple of a slab's bytes rounds down to whole slabs
        odd, _, _ = _case(gauss, (S,), rows, T, "1100 rows, C 300 -> 256", weights=w, values=dict(M=2, offset=True), infs=(True, True), scratch_bytes=300 * 8 * S)
        assert odd["info"]["rows_per_chunk"] == 256
        _same_bits(res["one chunk"], odd, "C 256")
        nodes = struct.unpack_from("<Q", gauss.stored[S].export_bart_state(), 28)[0]
        value = qc.device_bytes_formula(gauss.P, rows, nodes, S, gauss.T, True, 2, 0, 0, 384, 0) - 2 * 16          # (no quantiles per row, no probs there)
        want = sp.device_bytes_formula(value, rows, S, T, 384, weights=True, Q=len(PROBS))
        print(f"device memory of the call: {res['C 384']['info']['device_bytes']} bytes, the sum of DESIGN.md 5.14: {want}; the draws matrix would take {8 * rows * S}")
        assert res["C 384"]["info"]["device_bytes"] == want


# ---- the thresholds --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [0, 1, 5, 64])
def test_threshold_counts_and_the_two_bin_searches(gauss, T):
    rows, S = 300, 4
    infs = (T >= 5, T >= 5)
    res = {}
    for how in ("compare", "search", "auto"):
        res[how], (ref, bd), _ = _case(gauss, (S,), rows, T, f"T = {T}, {how}, no weights", values=dict(M=1), infs=infs, bin_index=how)
        assert res[how]["draws"].shape == (4 + 2 * T, S) and res[how]["quantiles"].shape == (len(PROBS), 4 + 2 * T)
    _same_bits(res["compare"], res["search"], f"T = {T}: the count of compares and the search")
    _same_bits(res["compare"], res["auto"], f"T = {T}: the library's choice")
    few, _, _ = _case(gauss, (S,), rows, T, f"T = {T}, C 128", values=dict(M=1), infs=infs, scratch_bytes=128 * 8 * S)
    _same_bits(res["auto"], few, f"T = {T}: one chunk and three")
    if T >= 5:          # t = -inf: every row lies above; t = +inf: none
        D = res["auto"]["draws"]
        assert np.all(D[4] == 1.0) and np.all(D[4 + T - 1] == 0.0) and np.all(D[4 + 2 * T - 1] == 0.0)
        r = sp.bound_ratio(D[4 + T], D[0], bd["draws"][4 + T] + bd["draws"][0])
        print(f"T = {T}: part_above at -inf against the mean: {r:.3g} x the sum of both bounds")
        assert r <= sp.BOUND_FACTOR
    w = np.random.default_rng(T).uniform(0.0, 2.0, rows)
    a, _, _ = _case(gauss, (S,), rows, T, f"T = {T}, compare, weights", weights=w, values=dict(M=1), infs=infs, bin_index="compare")
    b, _, _ = _case(gauss, (S,), rows, T, f"T = {T}, search, weights", weights=w, values=dict(M=1), infs=infs, bin_index="search", scratch_bytes=128 * 8 * S)
    _same_bits(a, b, f"T = {T}, weights: compares in one chunk and the search in three")


# ---- draw counts -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [(1,), (4,), (64, 1), (1, 64)])
def test_draw_counts(gauss, lens):
    rows, T = 300, 2
    got, _, _ = _case(gauss, lens, rows, T, f"{sum(lens)} draws {lens}", weights=np.random.default_rng(7).uniform(0.5, 1.5, rows), values=dict(M=1), scratch_bytes=128 * 8 * sum(lens))
    if sum(lens) == 1:
        assert np.all(got["m2"] == 0.0) and np.array_equal(got["mean"], got["draws"][:, 0])
    if lens == (1, 64):          # (64, 1)'s pooled draw k is (1, 64)'s draw perm[k]
        th = [0.0]
        other, _, _ = _case(gauss, (64, 1), rows, 1, "65 draws (64, 1), no tables", thresholds=th)
        mine, _, _ = _case(gauss, (1, 64), rows, 1, "65 draws (1, 64), no tables", thresholds=th)
        perm = np.r_[np.arange(1, 65), 0]
        assert np.array_equal(mine["draws"][:, perm], other["draws"]), "permuted peers: not the same values"
        assert np.array_equal(mine["quantiles"], other["quantiles"])


# ---- weights ---------------------------------------------------------------------------------------------------------------------------------------------
def test_weights_none_ones_a_slab_of_zeros_an_indicator_and_times_two(gauss):
    rows, S, T = 400, 9, 4
    values = dict(M=1, offset=True)
    none, _, call = _case(gauss, (S,), rows, T, "no weights", values=values, infs=(True, False))
    assert none["weight"] == float(rows) and np.all(none["draws"][4] == 1.0) and none["info"]["zero_slabs"] == 0
    th = call["thresholds"]
    ones, _, _ = _case(gauss, (S,), rows, T, "weights 1", weights=np.ones(rows), values=values, thresholds=th)
    _same_bits(none, ones, "no weights and weights 1")
    w = np.random.default_rng(3).uniform(0.5, 1.5, rows)
    w[128:256] = 0.0          # the second slab
    slab, _, call = _case(gauss, (S,), rows, T, "a slab of zero weights", weights=w, values=values, thresholds=th)
    assert slab["info"]["zero_slabs"] == 1
    twice = gauss.stored[S].predict_spread(**dict(call, weights=2.0 * w))
    assert twice["weight"] == 2.0 * slab["weight"]
    _same_bits(slab, twice, "weights times 2", keys=FLOATS)
    ind = (np.arange(rows) % 3 == 0).astype(np.float64)
    ind[:128] = 0.0           # the first slab: the first partial with weight is the second slab's
    one, _, call = _case(gauss, (S,), rows, T, "an indicator", weights=ind, values=values, thresholds=th)
    assert one["info"]["zero_slabs"] == 1 and np.all(one["draws"][4] == 1.0), "an indicator: share_above at -inf is not exactly 1"
    _same_bits(one, gauss.stored[S].predict_spread(**dict(call, weights=8.0 * ind)), "an indicator times 8", keys=FLOATS)
    dyadic = np.random.default_rng(4).integers(0, 17, rows) / 8.0
    dy, _, _ = _case(gauss, (S,), rows, T, "dyadic weights", weights=dyadic, values=values, thresholds=th)
    assert np.all(dy["draws"][4] == 1.0), "dyadic weights: share_above at -inf is not exactly 1"
    # the rows without weight do not reach the extremes
    keep = w > 0.0
    kw, x, bx = _values(gauss, (S,), rows, **values)
    assert np.all(np.abs(slab["draws"][2] - x[keep].min(axis=0).astype(np.float64)) <= sp.BOUND_FACTOR * bx.max(axis=0))


# ---- routes and samplers ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arms", [1, 2])
def test_routes_live_and_stored_two_calls(binary, arms):
    rows, S, T = 300, 13, 3
    values = dict(arms=arms, M=2, link=1, **(dict(col=binary.used_column(S), dense0=True) if arms == 2 else {}))
    w = np.random.default_rng(arms).uniform(0.0, 1.0, rows)
    res = {}
    for route in ("staged", "global"):
        res[route], _, call = _case(binary, (S,), rows, T, f"link 1, {arms} arm(s), {route}", weights=w, values=values, route=route)
        assert res[route]["info"]["route"] == (1 if route == "staged" else 2)
    _same_bits(res["staged"], res["global"], "the two routes")
    again = binary.stored[S].predict_spread(**call, route="global")
    _same_bits(res["global"], again, "two calls")
    live = binary.live.predict_spread(**call)
    _same_bits(res["staged"], live, "live and stored samplers")
    chunked = binary.live.predict_spread(**call, scratch_bytes=128 * 8 * S)
    _same_bits(res["staged"], chunked, "live, three chunks")


# ---- two arms under the identity link ---------------------------------------------------------------------------------------------------------------------
def test_two_arms_identity_link_and_no_affected_tree(gauss):
    rows, lens, T = 300, (9, 4), 3
    w = np.random.default_rng(2).uniform(0.0, 2.0, rows)
    col = gauss.used_column(9)
    a, _, _ = _case(gauss, lens, rows, T, "two arms, a BART column and a dense part", weights=w, values=dict(arms=2, M=2, col=col, dense0=True))
    assert a["info"]["route"] in (1, 2)
    b, _, call = _case(gauss, lens, rows, T, "two arms, a dense part only: no tree is walked", weights=w, values=dict(arms=2, M=2, dense0=True))
    assert b["info"]["route"] == 0, b["info"]
    c = gauss.stored[9].predict_spread(**call, scratch_bytes=128 * 8 * 13)
    _same_bits(b, c, "route 0: one chunk and three")


def test_swapped_arms_negate_bit_for_bit(gauss):
    """Swapping the arms negates every d bit for bit: the shift, s1 and so the mean and part_above at t = -inf change sign, min and max change places
    and sign, s2 and so sd are the same, share_above at -inf is the same."""
    rows, lens = 300, (9,)
    w = np.random.default_rng(5).uniform(0.0, 1.0, rows)
    values = dict(arms=2, M=2, col=gauss.used_column(9), dense0=True)
    a, _, _ = _case(gauss, lens, rows, 1, "two arms", weights=w, values=values, thresholds=[-np.inf])
    b, _, _ = _case(gauss, lens, rows, 1, "two arms, swapped", weights=w, values=dict(values, swap=True), thresholds=[-np.inf])
    A, B = a["draws"], b["draws"]
    assert np.any(A[0] != 0.0) and np.all(A[1] > 0.0)
    assert np.array_equal(B[0], -A[0]) and np.array_equal(B[2], -A[3]) and np.array_equal(B[3], -A[2]) and np.array_equal(B[5], -A[5]), "swapped arms do not negate bit for bit"
    assert np.array_equal(B[1], A[1]) and np.array_equal(B[4], A[4])
    assert b["mean"][0] == -a["mean"][0] and b["mean"][1] == a["mean"][1] and np.array_equal(b["m2"], a["m2"][[0, 1, 3, 2, 4, 5]])
    q0, q1 = PROBS.index(0.0), PROBS.index(1.0)
    assert b["quantiles"][q0, 0] == -a["quantiles"][q1, 0] and b["quantiles"][q1, 2] == -a["quantiles"][q0, 3] and np.array_equal(b["quantiles"][:, 1], a["quantiles"][:, 1])


# ---- cross-checks against shipped calls -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arms", [1, 2])
def test_the_mean_against_the_shipped_averages(gauss, arms):
    rows, lens = 1100, (9,)
    w = np.random.default_rng(9).uniform(0.0, 2.0, rows)
    values = dict(M=2, offset=True) if arms == 1 else dict(arms=2, M=2, col=gauss.used_column(9), dense0=True)
    got, (ref, bd), _ = _case(gauss, lens, rows, 1, f"{arms} arm(s) for the averages", weights=w, values=values, thresholds=[-np.inf])
    kw, x, bx = _values(gauss, lens, rows, **values)
    wn = w / got["weight"]
    args = {k: v for k, v in kw.items() if k not in ("n_arms", "peers", "peer_dense_coef")}
    if arms == 1:
        s = gauss.stored[9].predict_summary(weights=wn[None, :], **{k: v for k, v in args.items() if k not in ("x_test0", "dense0")})
    else:
        s = gauss.stored[9].predict_contrast(weights=wn[None, :], per_row=False, **args)
    # the shipped call adds the same terms, weighted by w / W, in another order: summary_cases' bound of its average, and the rounding of w / W
    b2 = wn @ bx + (rows + 1) * gc.U * (wn @ np.abs(x).astype(np.float64))
    r = gc.bound_ratio(got["draws"][0], s["average"][:, 0], bd["draws"][0] + b2)
    rp = gc.bound_ratio(got["draws"][5], got["draws"][0], bd["draws"][5] + bd["draws"][0])
    print(f"{arms} arm(s): the mean against the shipped average: {r:.3g} x the sum of both bounds; part_above at -inf against the mean: {rp:.3g}")
    assert r <= gc.BOUND_FACTOR and rp <= gc.BOUND_FACTOR


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(gauss):
    from stan4bart_amd.abi import SpreadIn, SpreadOut
    rows, S = 300, 9
    x = np.asfortranarray(gauss.x[:rows])
    live, smp = gauss.live, gauss.stored[S]

    def refused(match, **kw):
        before = live.get_counters()
        for s in (live, smp):
            args = dict(x_test=x, thresholds=(0.0,), probs=(0.5,))
            args.update(kw)
            with pytest.raises(RuntimeError, match=match):
                s.predict_spread(**args)
            assert not any(s.spread_info.values()), s.spread_info
        assert np.array_equal(live.get_counters(), before), "a refused call launched something"
    refused(r"predict_spread: n_thresholds must lie in \[0, 64\], not 65", thresholds=np.arange(65.0))
    refused("predict_spread: threshold 1 is a NaN", thresholds=(0.0, np.nan))
    refused("predict_spread: the thresholds are not strictly ascending at index 2", thresholds=(0.0, 1.0, 1.0))
    refused("predict_spread: the thresholds are not strictly ascending at index 1", thresholds=(np.inf, np.inf))
    refused("predict_spread: the thresholds are not strictly ascending at index 1", thresholds=(1.0, -1.0))
    for bad, name in ((-1.0, "-1"), (np.nan, "nan"), (np.inf, "inf")):
        w = np.ones(rows)
        w[17] = bad
        refused(f"predict_spread: weight {name}.* of row 17 is negative or not finite", weights=w)
    refused("predict_spread: the weights sum to 0", weights=np.zeros(rows))
    refused("predict_spread: n_arms must be 1 .* or 2 .*, not 3", n_arms=3)
    refused("predict_spread: n_arms = 1 takes no arm-0 pointer", x_test0=x)
    refused("predict_spread: bin_index must be 0 .*, not 3", bin_index=3)
    refused("predict_spread: prob 1.5.* outside", probs=(1.5,))
    # two weight vectors: the binding hands one down, so the struct is filled by hand

    def draws(s):
        return s.spread_draws()
    for s in (live, smp):
        before = live.get_counters()
        none = dict.fromkeys(("x_test0", "peer_dense_coef", "peer_ell_coef", "offset", "offset0", "dense", "dense0", "dense_coef", "ell_index", "ell_index0",
                              "ell_value", "ell_value0", "ell_coef"))
        arms, keep, _, G, _, _ = s._contrast_in(draws, x, probs=(), peers=(), link=0, weights=np.ones((2, rows)), route="auto", stage_nodes=0, scratch_bytes=0, **none)
        assert G == 2
        buf = np.zeros(4)
        out = SpreadOut(mean=buf.ctypes.data_as(C.POINTER(C.c_double)))
        out.info[0] = 7
        rc_ = s._f("predict_spread")(s._h, C.byref(SpreadIn(arms=arms, n_arms=1, n_thresholds=0, thresholds=None, bin_index=0)), C.byref(out))
        assert rc_ != 0 and not any(out.info) and np.all(buf == 0.0)
        with pytest.raises(RuntimeError, match="predict_spread: between 0 and 1 weight vectors, not 2"):
            s._check(rc_)
        assert np.array_equal(live.get_counters(), before)
        del keep
    ok = smp.predict_spread(x_test=x, thresholds=(0.0,), probs=(0.5,))
    assert ok["info"]["launches"] == 3 + 3, ok["info"]          # values, reduce, fold; finish, level rows, sort
    assert smp.predict_spread(x_test=x, outputs=("draws",))["info"]["launches"] == 3 + 1          # no summary asked for
    before = live.get_counters()
    live.predict_spread(x_test=x)
    assert live.get_counters()[2] == before[2] + 5


# ---- the Python interface --------------------------------------------------------------------------------------------------------------------------------
def test_whole_interface_and_bayes_r2(hip_lib):
    """Stan4bartFit.bayes_R2 against the same formula from fit.predict's matrix at 100 rows, and Stan4bartFit.predict_spread of the treatment effect
    against numpy over fit.predict of the two arms: weights, thresholds, chains pooled."""
    from stan4bart_amd import GroupTerm, generate_friedman_data
    from stan4bart_amd.abi import Sampler
    from stan4bart_amd.generics import combine_chains_f, stan4bart
    d = generate_friedman_data(120, ranef=True, causal=True, p=10)
    x, z = d["x"], np.asarray(d["z"], dtype=np.float64)
    xb, X = np.column_stack([x[:, [j for j in range(10) if j != 3]], z]), np.column_stack([x[:, 3], z])
    groups = [GroupTerm(d["g1"], None, "g.1"), GroupTerm(d["g2"], None, "g.2")]
    fit = stan4bart(d["y"], xb, X=X, groups=groups, chains=2, seed=99, iter=14, warmup=6, bart_args={"n.trees": 9, "keepTrees": True},
                    make_sampler=lambda a, st: Sampler(hip_lib, "s4b_", a, st))
    try:
        m = 100
        g = np.random.default_rng(11)
        xb1, X1, off = rc.new_rows(xb, m, seed=4), X[:m] + g.normal(size=(m, 2)), g.normal(size=m)
        new = [GroupTerm(np.asarray(d["g1"])[:m], None, "g.1"), GroupTerm(np.asarray(d["g2"])[:m], None, "g.2")]
        flat = combine_chains_f(fit.predict(x_bart=xb1, X=X1, groups=new, offset=off, combine_chains=False, seed=7))          # [rows x draws]
        sig = fit.stan[fit.par_names.index("aux.1")]
        sigma = np.concatenate([sig[:, c] for c in range(2)])
        v = flat.var(axis=0, ddof=1)
        want = v / (v + sigma ** 2)
        got = fit.bayes_R2(x_bart=xb1, X=X1, groups=new, offset=off, probs=(0.025, 0.975), seed=7)
        assert got["r2"].shape == (16,)
        np.testing.assert_allclose(got["r2"], want, rtol=1e-9)
        np.testing.assert_allclose([got["mean"], got["median"]], [want.mean(), np.median(want)], rtol=1e-9)
        np.testing.assert_allclose(got["quantiles"], np.quantile(want, (0.025, 0.975)), rtol=1e-9)
        # the treatment effect's spread
        w = g.uniform(0.0, 2.0, m)
        t1, t0 = xb1.copy(), xb1.copy()
        t1[:, 9], t0[:, 9] = 1.0, 0.0
        d1 = combine_chains_f(fit.predict(x_bart=t1, X=X1, groups=new, offset=off, combine_chains=False, seed=7))
        d0 = combine_chains_f(fit.predict(x_bart=t0, X=X1, groups=new, offset=off, combine_chains=False, seed=7))
        eff = d1 - d0
        th = (gc.midway(eff, 0.3), gc.midway(eff, 0.7))
        want = sp.brute_force(eff, w, th)
        probs = (0.025, 0.5, 0.975)
        full = fit.predict_spread(xb1, X=X1, groups=new, offset=off, treatment=("x_bart", 9), thresholds=th, row_weights=w, probs=probs, return_draws=True, seed=7)
        assert full["draws"] == 16 and full["names"] == sp.names(2) and np.isclose(full["weight"], w.sum()) and full["info"]["thresholds"] == 2
        np.testing.assert_allclose(full["matrix"], want, rtol=1e-8, atol=1e-11)
        np.testing.assert_allclose(full["effect_sd"], want[1], rtol=1e-8, atol=1e-11)
        np.testing.assert_allclose(full["mean"], want.mean(axis=1), rtol=1e-8, atol=1e-11)
        np.testing.assert_allclose(full["sd"], want.std(axis=1, ddof=1), rtol=1e-6, atol=1e-11)
        np.testing.assert_allclose(full["quantiles"], np.quantile(want, probs, axis=1), rtol=1e-8, atol=1e-11)
        with np.errstate(divide="ignore", invalid="ignore"):
            none = want[4:6] == 0.0
            np.testing.assert_allclose(full["mean_above"], np.where(none, np.nan, want[6:8] / want[4:6]), rtol=1e-8, atol=1e-11)
            np.testing.assert_allclose(full["gain"], np.where(none, np.nan, want[6:8] - np.array(th)[:, None] * want[4:6]), rtol=1e-8, atol=1e-11)
        brief = fit.predict_spread(xb1, X=X1, groups=new, offset=off, treatment=("x_bart", 9), thresholds=th, row_weights=w, probs=probs, seed=7)
        assert np.array_equal(brief["mean"], full["mean"]) and brief["effect_sd"]["mean"] == full["mean"][1]
        assert np.array_equal(brief["share_above"]["quantiles"], full["quantiles"][:, 4:6]) and "matrix" not in brief
    finally:
        fit.close()
