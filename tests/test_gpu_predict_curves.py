"""s4b_predict_curves on the device (stan4bart_amd/csrc/readout_curves.inc: k_curve_values<staged / global, cancelling or not>,
k_curve_rows, then the unchanged k_level_rows and k_row_quantiles) against the model of tests/curve_cases.py: predict_bart of the overwritten rows per
grid point, the linear parts and the link in long double, the derived bounds, and the sandwich of the p_max / p_min counts.  The cases are
curve_cases.CASES — rows 1, 63, 64, 65, 257; four chunks; 1, 2, 3, 4, 5 and 64 grid points; pooled draws 1, 7, 8, 9,
16, 17 and 70; a pair of predictors; anchor first, last and none; link 0 and a probit chain; offset, dense and ELL parts with another table per
pooled sampler — each on both routes, bit for bit; tests/test_predict_curves.py holds the ambiguity share of each
below 5 % on the CPU.  Bit for bit besides: two calls, live and stored samplers, any chunking, the shared points of a grid of 3 inside a grid of 9, a
permuted grid, the anchor's exact zero and the tie rule, an unused predictor.  To the bound besides: the row average of the means against
partial_dependence, the two-point anchored curve against predict_contrast.

The chains are tiny (n = 100 ... 300, 5 ... 20 trees, 13 kept draws); a model is computed once per case and shared by the routes."""
import os
import re

import numpy as np
import pytest

import curve_cases as cv
import pd_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CHAINS, _MODEL, WORST = {}, {}, {}


def _report(line):
    print(line)


@pytest.fixture(scope="module")
def chains(hip_lib):
    def get(kind):
        if kind not in _CHAINS:
            _CHAINS[kind] = cv.make_chain(hip_lib, "s4b_", kind)
        return _CHAINS[kind]
    yield get
    if WORST:
        k = max(WORST, key=WORST.get)
        print(f"largest device-to-model distance over the cases: {WORST[k]:.3g} of the bound ({k})")
    for c in _CHAINS.values():
        c.close()
    _CHAINS.clear()


def _call(chain, inp, pool=None, sampler=None, **kw):
    pool = inp["pool"] if pool is None else pool
    first = chain.stored[pool[0]] if sampler is None else sampler
    args = dict(inp["call"], probs=cv.PROBS, peers=[chain.stored[S] for S in pool[1:]])
    args.update(kw)
    return first.predict_curves(inp["x"], inp["vars"], inp["grid"], **args)


def _same(a, b, what):
    from stan4bart_amd.abi import CURVES_OUTPUTS
    for key in CURVES_OUTPUTS:
        assert np.array_equal(a[key], b[key]), f"{what}: {key} differs"


@pytest.mark.parametrize("name", sorted(cv.CASES))
def test_cases_against_the_model_on_both_routes(chains, name):
    case = cv.CASES[name]
    ch = chains(case["chain"])
    inp = cv.inputs(ch, case)
    if name not in _MODEL:
        _MODEL[name] = cv.case_model(ch, inp)
    ref, bd, extra = _MODEL[name]
    assert cv.ambiguity(ref, bd, extra) <= cv.AMBIGUOUS_MAX
    S, rows, G = sum(case["pool"]), case["rows"], case["G"]
    res = {}
    for route in ("staged", "global"):
        got = res[route] = _call(ch, inp, route=route)
        info = got["info"]
        assert got["draws"] == S and info["padded_draws"] >= S
        cancel = inp["anchor"] is not None and not inp["link"]
        hit = sum(ch.hit(s, inp["vars"]).sum() for s in case["pool"])
        assert info["total_affected"] == hit and info["largest_affected"] == max(ch.hit(s, inp["vars"]).sum(axis=1).max() for s in case["pool"])
        assert info["route"] == (0 if cancel and not hit else 1 if route == "staged" else 2), info
        want_c = cv.chunk_rows(rows, S, G, inp["call"]["scratch_bytes"])
        assert info["rows_per_chunk"] == want_c and info["chunks"] == -(-rows // want_c), info
        ratios = cv.assert_curves(got, ref, bd, extra, f"{name} {route}", _report)
        WORST[f"{name} {route}"] = max(ratios.values())
    _same(res["staged"], res["global"], f"{name}: the two routes")
    if case["scratch_rows"]:
        assert res["staged"]["info"]["chunks"] == 4
        _same(_call(ch, inp, scratch_bytes=0), res["staged"], f"{name}: one chunk against four")
    if inp["anchor"] is not None:          # the anchor's curve is exactly +0.0, and it wins every draw in which nothing lies above / below it
        a = inp["anchor"]
        got = res["staged"]
        for key in ("mean", "m2"):
            assert not got[key][:, a].any() and not np.signbit(got[key][:, a]).any()
        assert not got["quantiles"][:, :, a].any()


def test_two_calls_live_and_stored_samplers_and_peer_pools(chains):
    ch = chains("gauss")
    inp = cv.inputs(ch, cv._case(rows=130, G=6, pool=(13,), anchor="first", M=1, E=1, offset=True))
    a = _call(ch, inp)
    _same(_call(ch, inp), a, "two calls")
    _same(_call(ch, inp, sampler=ch.live), a, "live against stored")
    inp2 = cv.inputs(ch, cv._case(rows=130, G=6, pool=(13,), link=0))
    b = _call(ch, inp2, sampler=ch.live, anchor=None)
    _same(_call(ch, inp2, anchor=None), b, "live against stored, no anchor")
    assert ch.live.curves_draws() == 13 and b["draws"] == 13 and b["info"]["launches"] > 0


def test_shared_points_of_a_grid_inside_a_larger_one(chains):
    ch = chains("gauss")
    inp9 = cv.inputs(ch, cv._case(rows=100, G=9, pool=(5, 2), M=1))
    sub = [1, 4, 7]
    inp3 = dict(inp9, grid=np.asarray(inp9["grid"])[sub])
    for anchor9, anchor3 in ((None, None), (4, 1)):
        big, small = _call(ch, inp9, anchor=anchor9), _call(ch, inp3, anchor=anchor3)
        for key in ("mean", "m2"):
            assert np.array_equal(big[key][:, sub], small[key]), (key, anchor9)
        assert np.array_equal(big["quantiles"][:, :, sub], small["quantiles"]), anchor9


def test_a_permuted_grid_permutes_the_points_and_leaves_the_range(chains):
    ch = chains("gauss")
    inp = cv.inputs(ch, cv._case(rows=100, G=7, pool=(5, 2), E=1))
    perm = np.random.default_rng(5).permutation(7)
    for anchor in (None, 2):
        a = _call(ch, inp, anchor=anchor)
        b = _call(ch, dict(inp, grid=np.asarray(inp["grid"])[perm]), anchor=None if anchor is None else int(np.flatnonzero(perm == anchor)[0]))
        for key in ("mean", "m2"):
            assert np.array_equal(a[key][:, perm], b[key]), (key, anchor)
        assert np.array_equal(a["quantiles"][:, :, perm], b["quantiles"])
        for key in ("range_mean", "range_m2", "range_quantiles"):
            assert np.array_equal(a[key], b[key]), (key, anchor)
    # the shares move with their points in every row whose winners are certain and alone in their exact-tie class (the tie rule looks at the index):
    # one draw, so that a row's shares name its winners
    inp1 = cv.inputs(ch, cv._case(rows=257, G=7, pool=(1,), E=1))
    for anchor in (None, 2):
        a = _call(ch, inp1, anchor=anchor)
        b = _call(ch, dict(inp1, grid=np.asarray(inp1["grid"])[perm]), anchor=None if anchor is None else int(np.flatnonzero(perm == anchor)[0]))
        ref, bd, extra = cv.case_model(ch, dict(inp1, anchor=anchor), probs=())
        clean = cv.lone_winners(ref, bd, extra)
        _report(f"permuted grid, anchor {anchor}: {clean.sum()} of 257 rows have certain winners alone in their class")
        assert clean.sum() >= 5, "too few rows without an exact tie among the winners to say anything"
        for key in ("p_max", "p_min"):
            assert np.array_equal(a[key][clean][:, perm], b[key][clean]), (key, anchor)


def test_the_anchor_is_exactly_zero_and_ties_go_to_the_lowest_index(chains):
    ch = chains("gauss")
    inp = cv.inputs(ch, cv._case(rows=90, G=3, pool=(5, 2)))
    g = np.asarray(inp["grid"])
    inp["grid"] = np.r_[g[1], g, g[1]]          # points 0, 2 and 4 carry one value: one exact-tie class wherever they are
    for link, chain in ((0, ch), (1, chains("probit"))):
        if link:
            inp = cv.inputs(chain, cv._case(chain="probit", rows=90, G=3, pool=(5, 2), link=1))
            g = np.asarray(inp["grid"])
            inp["grid"] = np.r_[g[1], g, g[1]]
        for anchor in (0, 2, 4):
            got = _call(chain, inp, anchor=anchor)
            for a in (0, 2, 4):
                assert not got["mean"][:, a].any() and not got["m2"][:, a].any() and not got["quantiles"][:, :, a].any(), (link, anchor, a)
            assert not got["p_max"][:, [2, 4]].any() and not got["p_min"][:, [2, 4]].any(), "a later member of an exact-tie class won"
            ref, bd, extra = cv.case_model(chain, dict(inp, anchor=anchor))
            cv.assert_curves(got, ref, bd, extra, f"tie classes, link {link}, anchor {anchor}", _report)


def test_a_predictor_no_tree_splits_on(chains):
    ch = chains("unused")
    assert not ch.hit(13, 6).any()
    inp = cv.inputs(ch, cv._case(chain="unused", rows=100, G=5, pool=(5, 2), var=6, M=1))
    for anchor in (None, 3):
        for route in ("staged", "global"):
            got = _call(ch, inp, anchor=anchor, route=route)
            assert got["info"]["total_affected"] == 0 and got["info"]["route"] == (0 if anchor is not None else 1 if route == "staged" else 2)
            for key in ("range_mean", "range_m2", "range_quantiles"):
                assert not got[key].any(), key
            want = np.zeros((100, 5))
            want[:, 0] = 1.0
            assert np.array_equal(got["p_max"], want) and np.array_equal(got["p_min"], want)
            assert np.array_equal(got["mean"], np.repeat(got["mean"][:, :1], 5, axis=1))
            ref, bd, extra = cv.case_model(ch, dict(inp, anchor=anchor))
            cv.assert_curves(got, ref, bd, extra, f"unused predictor, anchor {anchor}, {route}", _report)


@pytest.mark.parametrize("link,kind", [(0, "gauss"), (1, "probit")])
def test_row_average_of_the_means_against_partial_dependence(chains, link, kind):
    """sum_i mean[i, g] / rows and the draw mean of partial_dependence's pd[k, g] are two device routes to one number: each within its own model's bound
    of it, plus the roundings of the two averages formed here (rows + S additions of numbers no larger than max |v|)."""
    ch = chains(kind)
    S, rows = 5, 120
    inp = cv.inputs(ch, cv._case(chain=kind, rows=rows, G=6, pool=(S,), link=link, M=1, offset=True))
    got = _call(ch, inp, anchor=None, outputs=("mean",), probs=())
    ref, bd, _ = cv.case_model(ch, inp, probs=())
    call = {k: inp["call"][k] for k in ("offset", "dense", "dense_coef", "ell_index", "ell_value", "ell_coef", "link")}
    pd = ch.stored[S].partial_dependence(inp["x"], inp["vars"], inp["grid"], **call)["pd"]
    pd_ref, pd_bound = ch.reference(S, rows, inp["vars"], inp["grid"], link=link, **{k: v for k, v in call.items() if k != "link"})
    np.testing.assert_allclose(pd_ref.mean(axis=0), ref["mean"].mean(axis=0), rtol=1e-12, atol=1e-13)          # the two models agree
    bound = bd["mean"].mean(axis=0) + pd_bound.mean(axis=0) + (rows + S) * cv.U * np.abs(ref["c"]).max()
    r = cv.bound_ratio(got["mean"].mean(axis=0), pd.mean(axis=0), bound)
    _report(f"row average of predict_curves' means against partial_dependence, link {link}: {r:.3g} of the bound")
    assert r <= cv.BOUND_FACTOR


def test_two_point_anchored_curve_against_predict_contrast(chains):
    ch = chains("gauss")
    inp = cv.inputs(ch, cv._case(rows=150, G=2, pool=(5, 2), anchor="first"))
    v = inp["vars"][0]
    # two grid values in different bins of the predictor: its column is then the one differing column of the contrast
    col = np.sort(np.asarray(ch.args.x_bart)[:, v])
    inp["grid"] = np.array([col[len(col) // 4], col[3 * len(col) // 4]])
    got = _call(ch, inp)
    x1, x0 = pc.overwritten(inp["x"], [v], [inp["grid"][1]]), pc.overwritten(inp["x"], [v], [inp["grid"][0]])
    con = ch.stored[5].predict_contrast(x1, x0, probs=cv.PROBS, peers=[ch.stored[2]])
    assert con["info"]["differing_columns"] == 1 and con["info"]["total_affected"] == got["info"]["total_affected"] > 0
    ref, bd, extra = cv.case_model(ch, inp)
    for key, mine in (("mean", got["mean"][:, 1]), ("m2", got["m2"][:, 1]), ("quantiles", got["quantiles"][:, :, 1])):
        r = cv.bound_ratio(con[key], ref[key][..., 1], bd[key][..., 1])
        assert r <= cv.BOUND_FACTOR, (key, r)
        _report(f"two-point anchored curve against predict_contrast: {key} bit-equal: {np.array_equal(con[key], mine)}; contrast within {r:.3g} of the curve model's bound")
        assert np.array_equal(con[key], mine), f"{key}: the same additions in the same order, but other bits"


def test_fit_method_pools_the_chains(chains, hip_lib):
    """Stan4bartFit.predict_curves over stand-in chains: one pooled call on the first sampler with the others as peers."""
    import summary_cases as sc
    ch = chains("gauss")
    fit, _, _ = sc.fake_fit(0, n_iter=5, n_chain=2, samplers=[ch.stored[5], ch.stored[5]])
    x = ch.x[:50]
    out = fit.predict_curves(cv.busiest(ch, 13), x, anchor=0, type="indiv.bart")
    G = len(out["grid"])
    assert out["draws"] == 10 and out["mean"].shape == out["sd"].shape == out["p_max"].shape == (50, G) and out["quantiles"].shape == (3, 50, G)
    assert out["range"]["quantiles"].shape == (3, 50) and np.all(out["range"]["mean"] >= 0) and np.allclose(out["p_max"].sum(axis=1), 1.0)
    direct = ch.stored[5].predict_curves(x, cv.busiest(ch, 13), out["grid"], anchor=0, probs=(0.025, 0.5, 0.975), peers=[ch.stored[5]])
    assert np.array_equal(direct["mean"], out["mean"]) and np.array_equal(direct["range_quantiles"], out["range"]["quantiles"])


def test_constants_of_the_cases_are_the_kernels():
    text = open(os.path.join(ROOT, "stan4bart_amd", "csrc", "readout_curves.inc")).read()
    assert "void k_curve_values(" in text and "void k_curve_rows(" in text
    assert {1, 2, 3, 4, 5, 64} <= {c["G"] for c in cv.CASES.values()}
    assert {sum(c["pool"]) for c in cv.CASES.values()} >= {1, 7, 8, 9, 16, 17, 70} and {c["rows"] for c in cv.CASES.values()} >= {1, 63, 64, 65, 257}
