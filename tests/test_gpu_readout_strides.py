"""The chunked read-outs on the device where a chunk outgrows one grid of tiles or one sort (tests/stride_cases.py: the shapes and what each reaches,
held on the CPU by tests/test_readout_strides.py).  1 048 641 rows in ONE chunk: workgroup 0 of k_predict_values, k_contrast_values and k_curve_values
takes a second tile, of 65 rows; the level matrix of predict_groups with every row its own level and the 3 145 923 curve rows of predict_curves go
through LevelsSummary::run in two and in four pieces, k_level_rows through its grid stride.  Every call runs on both routes, bit for bit the same,
against a call of the same rows in chunks of 2^18 (one trip, one piece), bit for bit the same, and against the models of quantile_cases, contrast_cases,
summary_cases and curve_cases; rows per chunk, chunks and launches are stride_cases' — the launch count is what shows that the pieces ran.

One chain for the module: readout_cases.PREDICT_CASES["cap-exact"]'s (n = 400, 5 trees, 8 kept draws), stored samplers of 2 and 1 draws pooled (S = 3),
the hard rows of its rules in front and new rows behind them."""
import numpy as np
import pytest

from stan4bart_amd.abi import CURVES_OUTPUTS

import contrast_cases as cc
import curve_cases as cv
import quantile_cases as qc
import readout_cases as rc
import stride_cases as st
import summary_cases as sc
import test_gpu_predict_contrast as tc

pytestmark = pytest.mark.gpu
ROUTES = ("staged", "global")
_QUANTILES = {}


def _report(line):
    print(line)


@pytest.fixture(scope="module")
def consts():
    return st.constants()


@pytest.fixture(scope="module")
def chain(hip_lib):
    c = st.make_chain(hip_lib, "s4b_", st.big_rows())
    yield c
    _QUANTILES.clear()
    c.close()


def _sizes(info, p, launches, what):
    assert (info["rows_per_chunk"], info["chunks"], info["launches"]) == (p["C"], p["chunks"], launches), (what, info, p["C"], p["chunks"], launches)


# ---- (a) predict_quantiles: k_predict_values, two tiles in one workgroup --------------------------------------------------------------------------------
def _quantile_inputs(chain, rows):
    """test_gpu_predict_quantiles._inputs over this chain: one dense column, one ELL entry, an offset; a table of its own per pooled sampler."""
    x = np.asfortranarray(chain.x[:rows])
    shared = sc.linear_parts(rows, st.POOL[0], 1, 1, seed=0)
    tables = [shared] + [sc.linear_parts(rows, s, 1, 1, seed=100 + j) for j, s in enumerate(st.POOL[1:])]
    off = 1e3 * float(chain.range[1] - chain.range[0]) * np.random.default_rng(0).uniform(-1.0, 1.0, rows)
    kw = dict(x_test=x, offset=off, peers=[chain.stored[s] for s in st.POOL[1:]], peer_dense_coef=[t["dense_coef"] for t in tables[1:]],
              peer_ell_coef=[t["ell_coef"] for t in tables[1:]], **shared)
    parts = [dict(bart=chain.bart(s, (rows,), x), dense_coef=t["dense_coef"], ell_coef=t["ell_coef"]) for s, t in zip(st.POOL, tables)]
    row_side = dict(offset=off, dense=shared["dense"], ell_index=shared["ell_index"], ell_value=shared["ell_value"])
    return kw, parts, row_side


def _quantiles(chain, consts):
    """The one-chunk predict_quantiles call on both routes, its inputs and the model (ref, bound, v, bound of v): computed once, shared by (a) and (c)."""
    if not _QUANTILES:
        N = st.big_rows(consts)
        kw, parts, row_side = _quantile_inputs(chain, N)
        _QUANTILES.update(kw=kw, model=qc.model(parts, st.PROBS, **row_side),
                          got={route: chain.stored[st.POOL[0]].predict_quantiles(probs=st.PROBS, route=route, **kw) for route in ROUTES})
    return _QUANTILES


def test_predict_quantiles_two_tiles_in_one_workgroup(chain, consts):
    N = st.big_rows(consts)
    q = _quantiles(chain, consts)
    p = st.plan(N, st.S, c=consts)
    assert p["trips_first"] == 2 and p["last_tile_rows"] == 65
    ref, bd, _, _ = q["model"]
    for route in ROUTES:
        got = q["got"][route]
        assert got["draws"] == st.S and got["info"]["route"] == (1 if route == "staged" else 2)
        _sizes(got["info"], p, st.quantiles_launches(p), f"one chunk, {route}")
        qc.assert_quantiles(got, ref, bd, f"{N} rows in one chunk, {route}", _report)
    one = q["got"]["staged"]["quantiles"]
    assert np.array_equal(one, q["got"]["global"]["quantiles"]), "the two routes differ"
    pc = st.plan(N, st.S, 1, st.compare_scratch(), c=consts)
    for route in ROUTES:
        chunked = chain.stored[st.POOL[0]].predict_quantiles(probs=st.PROBS, route=route, scratch_bytes=st.compare_scratch(), **q["kw"])
        _sizes(chunked["info"], pc, st.quantiles_launches(pc), f"chunks of 2^18, {route}")
        differ = np.flatnonzero((chunked["quantiles"] != one).any(axis=0))
        assert not len(differ), f"{route}: {len(differ)} rows differ between one chunk and chunks of 2^18, the first at row {differ[0]}"


# ---- (b) predict_contrast: k_contrast_values ------------------------------------------------------------------------------------------------------------
def test_predict_contrast_two_tiles_in_one_workgroup(chain, consts):
    N = st.big_rows(consts)
    cols = (max(range(chain.P), key=lambda j: sum(int(chain.counts(s, (j,)).sum()) for s in st.POOL)),)
    assert sum(int(chain.counts(s, cols).sum()) for s in st.POOL) > 0
    kw, parts, arm1, a0, w = tc._inputs(chain, st.POOL, N, cols, M=1, offset=True, arm0=("dense0",), G=2, seed=1)
    ref, bd = cc.model(parts, arm1, a0, chain.T, chain.range, chain.binary, weights=w, probs=st.PROBS)
    p, pc = st.plan(N, st.S, c=consts), st.plan(N, st.S, 1, st.compare_scratch(), c=consts)
    res = {}
    for route in ROUTES:
        got = res[route] = chain.stored[st.POOL[0]].predict_contrast(probs=st.PROBS, route=route, **kw)
        info = got["info"]
        assert got["draws"] == st.S and info["route"] == (1 if route == "staged" else 2) and info["differing_columns"] == 1
        _sizes(info, p, st.contrast_launches(p, True, 2, len(st.PROBS)), f"one chunk, {route}")
        cc.assert_contrast(got, ref, bd, f"{N} rows in one chunk, {route}", _report)
    assert tc._same_bits(res["staged"], res["global"]), "the two routes differ"
    for route in ROUTES:
        chunked = chain.stored[st.POOL[0]].predict_contrast(probs=st.PROBS, route=route, scratch_bytes=st.compare_scratch(), **kw)
        _sizes(chunked["info"], pc, st.contrast_launches(pc, True, 2, len(st.PROBS)), f"chunks of 2^18, {route}")
        for key in ("mean", "m2", "quantiles"):
            differ = np.flatnonzero((chunked[key] != res["staged"][key]).reshape(-1, N).any(axis=0))
            assert not len(differ), f"{route}: {key} of {len(differ)} rows differs between one chunk and chunks of 2^18, the first at row {differ[0]}"
        cc.assert_contrast(chunked, ref, bd, f"{N} rows in chunks of 2^18, {route}", _report, keys=("average",))          # (the fold over the chunks: another association)


# ---- (c) predict_groups, every row its own level: arm_values_launch, k_level_reduce, k_level_rows' grid stride, the sort in two pieces ------------------
def test_predict_groups_every_row_its_own_level(chain, consts):
    N = st.big_rows(consts)
    q = _quantiles(chain, consts)
    _, _, v, bv = q["model"]
    ref, bd = sc.summarise(v, bv)
    p = st.plan(N, st.S, c=consts)
    assert st.pieces(N, 1, consts)["pieces"] == 2
    level = np.arange(N)
    want = q["got"]["staged"]["quantiles"]
    res = {}
    for route in ROUTES:
        got = res[route] = chain.stored[st.POOL[0]].predict_groups(level=level, n_levels=N, statistic="sum", probs=st.PROBS, outputs=("mean", "m2", "draws"),
                                                                   presorted=True, route=route, **q["kw"])
        info = got["info"]
        assert got["draws_pooled"] == st.S and info["edge_levels"] == 0 and info["nan_levels"] == 0 and info["route"] == (1 if route == "staged" else 2)
        _sizes(info, p, st.groups_launches(p, N, probs=len(st.PROBS), c=consts), f"L = rows, {route}")
        assert info["launches"] == 5          # values, reduce, level rows, two sorts
        differ = np.flatnonzero((got["quantiles"] != want).any(axis=0))
        assert not len(differ), f"{route}: the quantiles of {len(differ)} levels are not predict_quantiles' of their row, the first at level {differ[0]}"
        # h = p (S - 1) is an integer for the three probs: predict_quantiles' result is the row's three values sorted, so the level matrix is held to
        # k_predict_values' own output bit for bit
        differ = np.flatnonzero((np.sort(got["draws"], axis=1) != want.T).any(axis=1))
        assert not len(differ), f"{route}: the draws of {len(differ)} levels are not the row's values, the first at level {differ[0]}"
        ratios = {key: rc.bound_ratio(got[key], ref[key], bd[key]) for key in ("mean", "m2")}
        _report(f"predict_groups L = {N} rows, {route}: max |device - model| / bound: " + ", ".join(f"{k} {r:.3g}" for k, r in ratios.items()))
        assert max(ratios.values()) <= rc.BOUND_FACTOR, ratios
    for key in ("mean", "m2", "draws", "quantiles"):
        assert np.array_equal(res["staged"][key], res["global"][key]), f"the two routes differ in {key}"


# ---- (d), (e) predict_curves: k_curve_values, k_curve_rows, LevelsSummary in pieces ---------------------------------------------------------------------
def _rows_of(got, sel):
    """The rows `sel` of a predict_curves result, in the result's layout."""
    out = {k: got[k] for k in ("info", "draws")}
    for key in CURVES_OUTPUTS:
        out[key] = got[key][:, sel] if key in ("quantiles", "range_quantiles") else got[key][sel]
    return out


def _curves(chain, consts, rows, G, anchor, scratch, what):
    """One shape of predict_curves with all outputs: one chunk on both routes against the model on the selected rows and against `scratch`-byte chunks."""
    sel = st.selection(rows, G, consts)
    inp = st.curve_inputs(chain, rows, G, anchor, M=0 if anchor is not None else 1, offset=anchor is None)
    ref, bd, extra = st.curve_model(chain, inp, sel)
    assert cv.ambiguity(ref, bd, extra) <= cv.AMBIGUOUS_MAX
    first = chain.stored[st.POOL[0]]
    default = st.default_scratch("curves", consts)
    p, pc = st.plan(rows, st.S, G, 0, default, consts), st.plan(rows, st.S, G, scratch, default, consts)
    assert pc["chunks"] > 1 and pc["point"]["pieces"] == 1 and pc["trips_first"] == 1
    hit = sum(int(chain.hit(s, inp["vars"]).sum()) for s in st.POOL)
    assert hit > 0
    res = {}
    for route in ROUTES:
        got = res[route] = first.predict_curves(inp["x"], inp["vars"], inp["grid"], probs=st.CURVE_PROBS, route=route, **inp["call"])
        info = got["info"]
        assert got["draws"] == st.S and info["route"] == (1 if route == "staged" else 2) and info["total_affected"] == hit
        _sizes(info, p, st.curves_launches(p, G, probs=len(st.CURVE_PROBS), c=consts), f"{what}, one chunk, {route}")
        cv.assert_curves(_rows_of(got, sel), ref, bd, extra, f"{what}, {len(sel)} of {rows} rows, {route}", _report)
    one = res["staged"]
    for key in CURVES_OUTPUTS:
        assert np.array_equal(one[key], res["global"][key]), f"{what}: the two routes differ in {key}"
    if anchor is not None:
        for key in ("mean", "m2"):
            assert not one[key][:, anchor].any()
        assert not one["quantiles"][:, :, anchor].any()
    for route in ROUTES:
        chunked = first.predict_curves(inp["x"], inp["vars"], inp["grid"], probs=st.CURVE_PROBS, route=route, scratch_bytes=scratch, **inp["call"])
        _sizes(chunked["info"], pc, st.curves_launches(pc, G, probs=len(st.CURVE_PROBS), c=consts), f"{what}, chunks of {pc['C']}, {route}")
        for key in CURVES_OUTPUTS:
            a, b = one[key], chunked[key]
            same = (a == b) if key not in ("quantiles", "range_quantiles") else (a == b).all(axis=0)
            differ = np.flatnonzero(~same.reshape(rows, -1).all(axis=1))
            assert not len(differ), f"{what}, {route}: {key} of {len(differ)} rows differs between one chunk and chunks of {pc['C']}, the first at row {differ[0]}"
    return p


@pytest.mark.parametrize("anchor", [None, 0], ids=["plain", "cancelling"])
def test_predict_curves_two_tiles_four_pieces(chain, consts, anchor):
    N = st.big_rows(consts)
    p = _curves(chain, consts, N, st.G_BIG, anchor, st.compare_scratch(st.G_BIG), f"G {st.G_BIG}, anchor {anchor}")
    assert p["trips_first"] == 2 and p["point"]["pieces"] == 4 and p["range"]["pieces"] == 2 and p["point"]["level_rounds"] == 128


def test_predict_curves_two_pieces_without_the_tile_stride(chain, consts):
    """The pieces alone: were they wrong, this would fail while the quantiles of the big shape, which have no pieces, stayed clean."""
    n = st.small_rows(consts)
    p = _curves(chain, consts, n, st.G_SMALL, None, 8 * st.S * st.G_SMALL * (1 << 16), f"G {st.G_SMALL}, no second trip")
    assert p["trips_first"] == 1 and p["point"]["pieces"] == 2 and p["point"]["edges"] == [(209715, 1)] and p["range"]["pieces"] == 1
