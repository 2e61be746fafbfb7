"""s4b_predict_check on the device (stan4bart_amd/csrc/readout_check.inc: k_predict_values unchanged, k_check_reduce, k_check_fold, k_check_finish,
k_level_rows and k_row_quantiles unchanged over the [(7 + T) x S] matrix) against numpy in long double on the full replicate matrix
(tests/check_cases.py: the replicate, the model, the bounds, the thresholds).  The smallest shapes at which the reduction can go wrong: 1, 127, 128,
129 and 1 100 rows, the last in 9 chunks of exactly one slab, in 3 and in 1 (the same bits); 1, 4 and 65 pooled draws (a second block of lanes with
one live lane, pooled from stored samplers of different lengths in both orders); T = 0 (no LDS), 1, 5, 31, 32 (where the library's choice turns
from compares to the search) and 64, -inf and +inf among finite thresholds, the count of compares and the search (the same bits); no weights, unit
weights (the same bits), random weights, a slab of zero weights, an indicator whose first slab is empty; with and without row_scale; both routes,
live and stored samplers, link 0 and link 1.  Bit for bit: one row gives mean = min = max and sd = m3 = 0, and the extremes of its mean over the
draws are predict_ppd's quantiles at probs 0 and 1 under the same key; weights times 2, sigma times 4 with row_scale over 4 change nothing;
disc_rep is the same for samplers with different trees; without weights share_above is count / n; another key changes D; rows without weight whose
z lies beyond the range of Phi under link 1 leave the matrix finite and unchanged.  The refusals before any
launch; the device bytes; Stan4bartFit.pp_check against predict's matrix plus the model's noise.

Small Friedman chains, as tests/test_gpu_predict_projection.py builds them (its Chain and its reference values are used as they are): n = 100, 5
trees, stored samplers of 1, 4, 9 and 64 draws; a binary chain (11 trees; 5 and 13 draws) for link 1.  No element of any case is ambiguous (asserted
from the reference alone).  Measured on an MI355X, the largest |device - model| / bound of the module: min and max 0.46 (their bound is the replicate's
own), disc_rep 0.24, disc_obs 0.18, mean 0.16, share_above 0.026, sd 8e-5, m3 5e-5, observed 0.022; over the draws mean 0.12, m2 0.022, quantiles
0.21 (allowed: 4)."""
import struct

import numpy as np
import pytest

import check_cases as ck
import quantile_cases as qc
import readout_cases as rc
import spread_cases as sp
from test_gpu_predict_projection import Chain, _values

pytestmark = pytest.mark.gpu
WORST = {}
PROBS = (0.025, 0.5, 0.975, 0.0, 1.0, 1.0 / 3.0)
FLOATS = ("draws", "mean", "m2", "quantiles", "observed")
KEY = 0x9E3779B97F4A7C15


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
    print("predict_check, largest |device - model| / bound of this module: " + ", ".join(f"{k} {r:.3g}" for k, r in WORST.items()))


@pytest.fixture(scope="module")
def binary(hip_lib):
    c = Chain(hip_lib, rc._binary(n=400, T=11, warmup=6, iter=19), rows=300, steps=(1, 1, 3, 8))
    yield c
    c.close()


def _sigmas(lens):
    """One sigma vector per pooled sampler, by its position and length."""
    return [np.random.default_rng(100 + j).uniform(0.5, 1.5, S) for j, S in enumerate(lens)]


def _inputs(chain, lens, rows, link=0, values=None, scaled=True):
    """The keyword arguments of a pooled call over the first `rows` rows, and z, bz, the pooled sigma, y, row_scale of the model."""
    kw, z, bz = _values(chain, lens, rows, **(values or {}))
    kw = {k: v for k, v in kw.items() if k != "n_arms"}
    zf = np.asarray(z, dtype=np.float64)
    bz = np.broadcast_to(bz, zf.shape) + ck.U * np.abs(zf)          # (the reference z rounded to double)
    g = np.random.default_rng(rows + 7 * link)
    if link:
        y, rs, sig = (g.uniform(size=rows) < 0.5).astype(np.float64), None, None
        kw.update(link=1, y=y)
    else:
        y, rs, sig = zf[:, 0] + g.normal(size=rows), (g.uniform(0.5, 2.0, rows) if scaled else None), _sigmas(lens)
        kw.update(link=0, y=y, sigma=sig[0], peer_sigma=sig[1:] if len(lens) > 1 else None, row_scale=rs)
    return kw, zf, bz, (None if link else np.concatenate(sig)), y, rs


def _case(chain, lens, rows, T, what, link=0, weights=None, probs=PROBS, values=None, infs=(False, False), thresholds=None, sampler=None, key=KEY,
          scaled=True, **call):
    """One pooled call through the C-ABI against the model.  The finite thresholds lie midway between adjacent reference replicate values."""
    kw, z, bz, sigma, y, rs = _inputs(chain, lens, rows, link, values, scaled)
    if thresholds is None:
        thresholds = sp.thresholds_for(ck.replicate(z, bz, sigma, key, rs, link)["x"], T, *infs) if T else np.zeros(0)
    th = np.asarray(thresholds, dtype=np.float64)
    ref, bd = ck.model(z, bz, y, sigma, key, weights, th, probs, rs, link)
    got = (sampler or chain.stored[lens[0]]).predict_check(thresholds=th, weights=weights, probs=probs, noise_key=key, **kw, **call)
    S, info = sum(lens), got["info"]
    assert got["draws_pooled"] == S and info["draws"] == S and got["names"] == ck.names(len(th)) and got["draws"].shape == (7 + len(th), S), info
    _note(ck.assert_check(got, ref, bd, what, _report, weighted=weights is not None))
    return got, (ref, bd), dict(kw, thresholds=th, weights=weights, probs=probs, noise_key=key)


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
        res[name], _, call = _case(gauss, (S,), rows, T if rows > 1 else 2, f"{rows} rows, {name}", weights=w, values=dict(M=2, offset=True), infs=(True, True),
                                   scratch_bytes=Cr * 8 * S)
        info = res[name]["info"]
        want = min(rows, Cr) if Cr else rows
        assert info["rows_per_chunk"] == want and info["chunks"] == -(-rows // want) and info["launches"] == 3 * info["chunks"] + 3, info
    _same_bits(res["C 128"], res["C 384"], f"{rows} rows: C 128 and C 384")
    _same_bits(res["C 128"], res["one chunk"], f"{rows} rows: C 128 and one chunk")
    D = res["one chunk"]["draws"]
    Tn = len(call["thresholds"])
    assert np.all(D[5] <= 1.0 + 1e-12) and np.all(D[5 + Tn - 1] == 0.0), "t = +inf: not exactly 0"
    if rows == 1:          # one row: its replicate, no spread; the same replicate as predict_ppd's under the same key
        assert np.array_equal(D[0], D[3]) and np.array_equal(D[3], D[4]) and np.all(D[1] == 0.0) and np.all(D[2] == 0.0) and np.all(D[5] == 1.0)
        obs = res["one chunk"]["observed"]
        assert obs[0] == call["y"][0] == obs[3] == obs[4] and obs[1] == 0.0 and obs[2] == 0.0
        ppd = gauss.stored[S].predict_ppd(probs=(0.0, 1.0), noise_key=KEY, **{k: v for k, v in call.items() if k not in ("thresholds", "weights", "probs", "noise_key", "y")})
        assert ppd["quantiles"][0, 0] == D[0].min() and ppd["quantiles"][1, 0] == D[0].max(), "one row: not predict_ppd's replicate under the same key"
    if rows == 1100:
        assert [res[k]["info"]["chunks"] for k in ("C 128", "C 384", "one chunk")] == [9, 3, 1]
        nodes = struct.unpack_from("<Q", gauss.stored[S].export_bart_state(), 28)[0]
        value = qc.device_bytes_formula(gauss.P, rows, nodes, S, gauss.T, True, 2, 0, 0, 384, 0) - 2 * 16          # (no quantiles per row, no probs there)
        want = ck.device_bytes_formula(value, rows, S, T, 384, weights=True, row_scale=True, Q=len(PROBS))
        print(f"device memory of the call: {res['C 384']['info']['device_bytes']} bytes, the sum of DESIGN.md 5.15: {want}; the replicate matrix would take {8 * rows * S}")
        assert res["C 384"]["info"]["device_bytes"] == want


# ---- the thresholds --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [0, 1, 5, 31, 32, 64])
def test_threshold_counts_and_the_two_bin_routes(gauss, T):
    rows, S = 300, 4
    infs = (T >= 5, T >= 5)
    res = {}
    for how in ("compare", "search", "auto"):
        res[how], _, _ = _case(gauss, (S,), rows, T, f"T = {T}, {how}, no weights", values=dict(M=1), infs=infs, bin_index=how, scaled=False)
        assert res[how]["draws"].shape == (7 + T, S) and res[how]["quantiles"].shape == (len(PROBS), 7 + T) and res[how]["observed"].shape == (5 + T,)
    _same_bits(res["compare"], res["search"], f"T = {T}: the count of compares and the search")
    _same_bits(res["compare"], res["auto"], f"T = {T}: the library's choice")
    few, _, _ = _case(gauss, (S,), rows, T, f"T = {T}, C 128", values=dict(M=1), infs=infs, scratch_bytes=128 * 8 * S, scaled=False)
    _same_bits(res["auto"], few, f"T = {T}: one chunk and three")
    if T >= 5:          # t = -inf: every row lies above; t = +inf: none
        D = res["auto"]["draws"]
        assert np.all(D[5] == 1.0) and np.all(D[5 + T - 1] == 0.0)
        assert res["auto"]["observed"][5] == 1.0 and res["auto"]["observed"][5 + T - 1] == 0.0
    w = np.random.default_rng(T).uniform(0.0, 2.0, rows)
    a, _, _ = _case(gauss, (S,), rows, T, f"T = {T}, compare, weights", weights=w, values=dict(M=1), infs=infs, bin_index="compare")
    b, _, _ = _case(gauss, (S,), rows, T, f"T = {T}, search, weights", weights=w, values=dict(M=1), infs=infs, bin_index="search", scratch_bytes=128 * 8 * S)
    _same_bits(a, b, f"T = {T}, weights: compares in one chunk and the search in three")


# ---- draw counts -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [(1,), (4,), (64, 1), (1, 64)])
def test_draw_counts(gauss, lens):
    rows, T = 300, 2
    got, _, _ = _case(gauss, lens, rows, T, f"{sum(lens)} draws {lens}", weights=np.random.default_rng(7).uniform(0.5, 1.5, rows), values=dict(M=1),
                      scratch_bytes=128 * 8 * sum(lens))
    if sum(lens) == 1:
        assert np.all(got["m2"] == 0.0) and np.array_equal(got["mean"], got["draws"][:, 0])


def test_disc_rep_does_not_depend_on_the_trees_and_another_key_changes_the_matrix(gauss):
    """e belongs to (key, row of the call, pooled draw): the pools (9, 1) and (1, 9) hold different trees at every pooled draw, and the same
    discrepancy of the replicate, bit for bit (link 0)."""
    rows = 300
    w = np.random.default_rng(8).uniform(0.0, 2.0, rows)
    a, _, _ = _case(gauss, (9, 1), rows, 0, "the pool (9, 1)", weights=w)
    b, _, _ = _case(gauss, (1, 9), rows, 0, "the pool (1, 9)", weights=w)
    assert np.array_equal(a["draws"][5], b["draws"][5]), "disc_rep depends on the trees"
    assert not np.array_equal(a["draws"][0], b["draws"][0]) and not np.array_equal(a["draws"][6], b["draws"][6])
    c, _, _ = _case(gauss, (9, 1), rows, 0, "the pool (9, 1), another key", weights=w, key=KEY + 1)
    assert np.array_equal(a["draws"][6], c["draws"][6]) and np.array_equal(a["observed"], c["observed"]), "disc_obs or observed depends on the key"
    assert np.all(a["draws"][0] != c["draws"][0]) and np.all(a["draws"][5] != c["draws"][5]), "another key does not change the replicate"


# ---- weights and scales ----------------------------------------------------------------------------------------------------------------------------------
def test_weights_none_ones_a_slab_of_zeros_an_indicator_times_two_and_the_scales(gauss):
    rows, S, T = 400, 9, 4
    values = dict(M=1, offset=True)
    none, (ref, _), call = _case(gauss, (S,), rows, T, "no weights", values=values, infs=(True, False))
    assert none["weight"] == float(rows) and np.all(none["draws"][5] == 1.0) and none["info"]["zero_slabs"] == 0
    th = call["thresholds"]
    counts = (ref["x"][:, :, None] > th[None, None, :]).sum(axis=0).T
    assert np.array_equal(none["draws"][5:5 + T], counts / float(rows)), "without weights share_above is not count / n exactly"
    ones, _, _ = _case(gauss, (S,), rows, T, "weights 1", weights=np.ones(rows), values=values, thresholds=th)
    _same_bits(none, ones, "no weights and weights 1")
    w = np.random.default_rng(3).uniform(0.5, 1.5, rows)
    w[128:256] = 0.0          # the second slab
    slab, _, call = _case(gauss, (S,), rows, T, "a slab of zero weights", weights=w, values=values, thresholds=th)
    assert slab["info"]["zero_slabs"] == 1
    twice = gauss.stored[S].predict_check(**dict(call, weights=2.0 * w))
    assert twice["weight"] == 2.0 * slab["weight"]
    _same_bits(slab, twice, "weights times 2", keys=FLOATS)
    scaled = gauss.stored[S].predict_check(**dict(call, sigma=4.0 * call["sigma"], row_scale=call["row_scale"] / 4.0))
    _same_bits(slab, scaled, "sigma times 4, row_scale over 4")
    ind = (np.arange(rows) % 3 == 0).astype(np.float64)
    ind[:128] = 0.0           # the first slab: the first partial with weight is the second slab's
    one, _, call = _case(gauss, (S,), rows, T, "an indicator", weights=ind, values=values, thresholds=th)
    assert one["info"]["zero_slabs"] == 1 and np.all(one["draws"][5] == 1.0), "an indicator: share_above at -inf is not exactly 1"
    _same_bits(one, gauss.stored[S].predict_check(**dict(call, weights=8.0 * ind)), "an indicator times 8", keys=FLOATS)
    plain, _, _ = _case(gauss, (S,), rows, T, "no row_scale", weights=w, values=values, thresholds=th, scaled=False)
    assert not np.array_equal(plain["draws"][0], slab["draws"][0])
    unit = gauss.stored[S].predict_check(**dict(call, weights=w, row_scale=np.ones(rows)))
    _same_bits(plain, unit, "no row_scale and row_scale 1")


# ---- routes and samplers ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", [0, 1])
def test_routes_live_and_stored_two_calls(gauss, binary, link):
    chain, S = (binary, 13) if link else (gauss, 64)
    rows, T = 300, 0 if link else 3
    w = np.random.default_rng(link).uniform(0.0, 1.0, rows)
    res = {}
    for route in ("staged", "global"):
        res[route], _, call = _case(chain, (S,), rows, T, f"link {link}, {route}", link=link, weights=w, route=route)
        assert res[route]["info"]["route"] == (1 if route == "staged" else 2)
    _same_bits(res["staged"], res["global"], "the two routes")
    again = chain.stored[S].predict_check(**call, route="global")
    _same_bits(res["global"], again, "two calls")
    live = chain.live.predict_check(**call)
    _same_bits(res["staged"], live, "live and stored samplers")
    chunked = chain.live.predict_check(**call, scratch_bytes=128 * 8 * S)
    assert chunked["info"]["chunks"] == 3
    _same_bits(res["staged"], chunked, "live, three chunks")
    if link:
        D = res["staged"]["draws"]
        assert np.all((D[3] == 0.0) | (D[3] == 1.0)) and np.all((D[4] == 0.0) | (D[4] == 1.0)) and np.all((D[0] >= 0.0) & (D[0] <= 1.0))


@pytest.mark.parametrize("rows", [1, 129])
@pytest.mark.parametrize("lens", [(5,), (13, 1)])
def test_binary_replicate_at_slab_edges_and_pooled(binary, rows, lens):
    got, (ref, _), _ = _case(binary, lens, rows, 0, f"link 1, {rows} rows, {lens}", link=1, scratch_bytes=128 * 8 * sum(lens))
    assert ref["ambiguous"] == 0
    np.testing.assert_allclose(got["draws"][0], ref["x"].sum(axis=0) / float(rows), rtol=1e-13, atol=0.0)          # (the share of ones: the model's, assert_check)
    if rows == 1:
        D = got["draws"]
        assert np.array_equal(D[0], D[3]) and np.array_equal(D[3], D[4]) and np.all(D[1] == 0.0) and np.all(D[2] == 0.0)


def test_a_row_without_weight_beyond_the_range_of_phi_adds_no_nan(binary):
    """Under link 1 log Phi(+-z) is -inf from |z| of about 38 on.  A row of weight 0 adds no term to the discrepancy sums, so the matrix stays
    finite and is, bit for bit, the matrix of the call in which those rows have an ordinary z; with weight the deviance is +inf, its value."""
    rows, S = 130, 13
    x = np.asfortranarray(binary.x[:rows])
    y = (np.arange(rows) % 2).astype(np.float64)
    w = np.ones(rows)
    w[[5, 129]] = 0.0
    far = np.zeros(rows)
    far[5], far[129] = 60.0, -60.0
    smp = binary.stored[S]
    plain = smp.predict_check(x_test=x, y=y, link=1, weights=w, offset=np.zeros(rows), noise_key=KEY, probs=(0.5,))
    got = smp.predict_check(x_test=x, y=y, link=1, weights=w, offset=far, noise_key=KEY, probs=(0.5,), scratch_bytes=128 * 8 * S)
    assert np.all(np.isfinite(got["draws"])) and np.all(np.isfinite(got["mean"])) and np.all(np.isfinite(got["quantiles"]))
    _same_bits(plain, got, "rows without weight far outside the range of Phi")
    heavy = smp.predict_check(x_test=x, y=y, link=1, offset=far, noise_key=KEY)
    assert not np.any(np.isnan(heavy["draws"])) and np.all(np.isinf(heavy["draws"][6])) and np.all(heavy["draws"][6] > 0.0)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(gauss, binary):
    rows, S = 300, 9
    x = np.asfortranarray(gauss.x[:rows])
    y = np.random.default_rng(0).normal(size=rows)

    def refused(match, chain=gauss, **kw):
        live, smp = chain.live, chain.stored[S if chain is gauss else 13]
        before = live.get_counters()
        for s in (live, smp):
            args = dict(x_test=np.asfortranarray(chain.x[:rows]), y=y, sigma=np.ones(s.check_draws()), thresholds=(0.0,), probs=(0.5,))
            args.update(kw)
            with pytest.raises(RuntimeError, match=match):
                s.predict_check(**args)
            assert not any(s.check_info.values()), s.check_info
        assert np.array_equal(live.get_counters(), before), "a refused call launched something"
    refused(r"predict_check: n_thresholds must lie in \[0, 64\], not 65", thresholds=np.arange(65.0))
    refused("predict_check: n_thresholds must be 0 under link 1", chain=binary, link=1, sigma=None, y=np.arange(float(rows)) % 2)
    refused("predict_check: y holds 2.* under link 1 every y is 0 or 1", chain=binary, link=1, sigma=None, thresholds=(), y=np.arange(float(rows)) % 3)
    refused("predict_check: threshold 1 is a NaN", thresholds=(0.0, np.nan))
    refused("predict_check: the thresholds are not strictly ascending at index 2", thresholds=(0.0, 1.0, 1.0))
    refused("predict_check: the thresholds are not strictly ascending at index 1", thresholds=(np.inf, np.inf))
    for bad, name in ((-1.0, "-1"), (np.nan, "nan"), (np.inf, "inf")):
        w = np.ones(rows)
        w[17] = bad
        refused(f"predict_check: weight {name}.* of row 17 is negative or not finite", weights=w)
    refused("predict_check: the weights sum to 0", weights=np.zeros(rows))
    refused("predict_check: bin_index must be 0 .*, not 3", bin_index=3)
    refused("predict_check: prob 1.5.* outside", probs=(1.5,))
    refused("predict_check: NULL y", y=None)
    refused("predict_check: link 0 needs sigma", sigma=None)
    bad = np.ones(rows)
    bad[3] = np.nan
    refused("predict_check: y holds nan.* at row 3", y=bad)
    bad = np.ones(rows)
    bad[5] = 0.0
    refused("predict_check: row_scale is 0 at row 5", row_scale=bad)
    smp, live = gauss.stored[S], gauss.live
    ok = smp.predict_check(x_test=x, y=y, sigma=np.ones(S), thresholds=(0.0,), probs=(0.5,))
    assert ok["info"]["launches"] == 3 + 3, ok["info"]          # values, reduce, fold; finish, level rows, sort
    assert smp.predict_check(x_test=x, y=y, sigma=np.ones(S), outputs=())["info"]["launches"] == 3 + 1          # no summary asked for
    before = live.get_counters()
    live.predict_check(x_test=x, y=y, sigma=np.ones(64))
    assert live.get_counters()[2] == before[2] + 5


# ---- the Python interface --------------------------------------------------------------------------------------------------------------------------------
def test_whole_interface_pp_check(hip_lib):
    """Stan4bartFit.pp_check against the same statistics from fit.predict(type="ev")'s matrix plus the model's noise at 100 rows: the matrix, the
    summaries, observed and the p-values; the same seed gives predict_ppd's replicate."""
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
        xb1, X1 = xb[:m], X[:m]
        new = [GroupTerm(np.asarray(d["g1"])[:m], None, "g.1"), GroupTerm(np.asarray(d["g2"])[:m], None, "g.2")]
        y = np.asarray(d["y"], dtype=np.float64)[:m]
        ev = combine_chains_f(fit.predict(x_bart=xb1, X=X1, groups=new, combine_chains=False, seed=7))          # [rows x draws]
        sig = fit.stan[fit.par_names.index("aux.1")]
        sigma = np.concatenate([sig[:, c] for c in range(2)])
        w, ow = g.uniform(0.0, 2.0, m), g.uniform(0.5, 2.0, m)
        probs = (0.025, 0.5, 0.975)
        first = fit.pp_check(x_bart=xb1, X=X1, groups=new, y=y, seed=7)
        key = first["noise_key"]
        e, _ = ck.ppd.noise(key, np.arange(m), np.arange(16))
        e = e.astype(np.float64)
        sd = sigma[None, :] / np.sqrt(ow)[:, None]
        yrep = ev + sd * e
        th = (ck.gc.midway(yrep, 0.3), ck.gc.midway(yrep, 0.7))
        full = fit.pp_check(x_bart=xb1, X=X1, groups=new, y=y, thresholds=th, row_weights=w, obs_weights=ow, probs=probs, seed=7, return_draws=True)
        assert full["noise_key"] == key and full["seed"] == 7 and full["draws"] == 16 and full["names"] == ck.names(2) and np.isclose(full["weight"], w.sum())
        want = ck.brute_force(yrep, w, th)
        disc = np.vstack([(w[:, None] * e * e).sum(axis=0), (w[:, None] * ((y[:, None] - ev) / sd) ** 2).sum(axis=0)]) / w.sum()
        D = full["matrix"]
        np.testing.assert_allclose(D[:7], want, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(D[7:], disc, rtol=1e-8)
        obs = ck.brute_force(y[:, None], w, th)[:, 0]
        views = [full["mean"], full["sd"], None, full["min"], full["max"]] + full["share_above"]
        for mrow, v in enumerate(views):
            if v is None:
                continue
            np.testing.assert_allclose(v["observed"], obs[mrow], rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose([v["mean"], v["sd"]], [want[mrow].mean(), want[mrow].std(ddof=1)], rtol=1e-6, atol=1e-11)
            np.testing.assert_allclose(v["quantiles"], np.quantile(want[mrow], probs), rtol=1e-8, atol=1e-10)
            assert v["p_value"] == np.mean(want[mrow] >= obs[mrow]) and np.array_equal(v["draws"], D[mrow])
        sk = want[2] / want[1] ** 3
        np.testing.assert_allclose(full["skewness"]["draws"], sk, rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(full["skewness"]["observed"], obs[2] / obs[1] ** 3, rtol=1e-8)
        assert full["skewness"]["p_value"] == np.mean(sk >= obs[2] / obs[1] ** 3)
        assert full["discrepancy"]["p_value"] == np.mean(disc[0] >= disc[1]) and np.array_equal(full["discrepancy"]["draws_obs"], D[8])
        # the interval of the same seed speaks of the same replicate
        ppd = fit.predict_ppd(x_bart=xb1[:1], X=X1[:1], groups=[GroupTerm(np.asarray(d["g1"])[:1], None, "g.1"), GroupTerm(np.asarray(d["g2"])[:1], None, "g.2")],
                              probs=(0.0, 1.0), obs_weights=ow[:1], seed=7)
        one = fit.pp_check(x_bart=xb1[:1], X=X1[:1], groups=[GroupTerm(np.asarray(d["g1"])[:1], None, "g.1"), GroupTerm(np.asarray(d["g2"])[:1], None, "g.2")],
                           y=y[:1], obs_weights=ow[:1], seed=7, return_draws=True)
        assert ppd["noise_key"] == one["noise_key"] and ppd["quantiles"][0, 0] == one["mean"]["draws"].min() and ppd["quantiles"][1, 0] == one["mean"]["draws"].max()
        brief = fit.pp_check(x_bart=xb1, X=X1, groups=new, y=y, thresholds=th, row_weights=w, obs_weights=ow, probs=probs, seed=7)
        assert brief["mean"]["mean"] == full["mean"]["mean"] and "matrix" not in brief and "draws" not in brief["sd"]
    finally:
        fit.close()
