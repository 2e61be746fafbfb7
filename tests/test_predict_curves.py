"""s4b_predict_curves without a GPU: the model of tests/curve_cases.py against a brute-force numpy loop over the emulated layer's predict_bart; the share
of ambiguous (row, draw) pairs of EVERY case the GPU tests run, from the model alone (the sandwich of p_max / p_min must not go vacuous); the chunk-size
rule restated; every refusal of the argument checks, which run on every device layer before anything is launched; the launch refusal of the emulated
layer (no curve kernels there); the entry's absence from the oracle library and its presence in the header.  The kernels are tested in
tests/test_gpu_predict_curves.py."""
import os
import re

import numpy as np
import pytest

import curve_cases as cv
import pd_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CHAINS = {}


@pytest.fixture(scope="module")
def chains(emul_lib):
    def get(kind):
        if kind not in _CHAINS:
            _CHAINS[kind] = cv.make_chain(emul_lib, "emu_", kind)
        return _CHAINS[kind]
    yield get
    for c in _CHAINS.values():
        c.close()
    _CHAINS.clear()


@pytest.mark.parametrize("anchor", [None, 0, 3])
def test_model_against_a_brute_force_loop(chains, anchor):
    ch = chains("gauss")
    inp = cv.inputs(ch, cv._case(rows=40, G=4, pool=(2, 1)))
    inp["anchor"] = anchor
    ref, bd, extra = cv.case_model(ch, inp)
    x, vs, grid = inp["x"], inp["vars"], inp["grid"]
    want = np.concatenate([cv.brute_force(ch.stored[S].predict_bart, x, vs, grid, anchor) for S in inp["pool"]], axis=2)
    assert ref["c"].shape == want.shape == (40, 4, 3)
    np.testing.assert_allclose(ref["c"].astype(np.float64), want, rtol=0, atol=1e-13)
    np.testing.assert_allclose(ref["mean"], want.mean(axis=2), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(ref["m2"], ((want - want.mean(axis=2, keepdims=True)) ** 2).sum(axis=2), rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(ref["quantiles"], np.quantile(want, cv.PROBS, axis=2), rtol=1e-10, atol=1e-13)
    r = want.max(axis=1) - want.min(axis=1)
    np.testing.assert_allclose(ref["r"].astype(np.float64), r, rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(ref["range_mean"], r.mean(axis=1), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(ref["range_quantiles"], np.quantile(r, cv.PROBS, axis=1), rtol=1e-10, atol=1e-13)
    assert all(np.all(b >= 0) for b in bd.values())
    if anchor is not None:
        assert not ref["c"][:, anchor].any() and not bd["c"][:, anchor].any()          # the anchor: exactly 0, no allowance
    # the counts against the plain argmax where nothing is ambiguous
    cmax, pmax, cmin, pmin, amb = cv.counts(ref["c"], bd["c"], extra["sig"])
    assert np.all(cmax <= pmax) and np.all(cmin <= pmin)
    first_max = np.stack([(want.argmax(axis=1) == g).sum(axis=1) for g in range(4)], axis=1)          # numpy's argmax: the lowest index on a tie
    first_min = np.stack([(want.argmin(axis=1) == g).sum(axis=1) for g in range(4)], axis=1)
    assert np.all(cmax <= first_max) and np.all(first_max <= pmax) and np.all(cmin <= first_min) and np.all(first_min <= pmin)


def test_tie_classes_follow_the_leaves_and_the_lowest_index_wins(chains):
    ch = chains("gauss")
    inp = cv.inputs(ch, cv._case(rows=30, G=3, pool=(5,)))
    g = np.asarray(inp["grid"])
    inp["grid"] = np.r_[g[1], g, g[1]]          # points 0, 2 and 4 are one value: equal bins, one exact-tie class
    ref, bd, extra = cv.case_model(ch, inp)
    sig = extra["sig"]
    assert np.array_equal(sig[:, 0], sig[:, 2]) and np.array_equal(sig[:, 0], sig[:, 4]) and np.array_equal(ref["c"][:, 0], ref["c"][:, 4])
    cmax, pmax, cmin, pmin, _ = cv.counts(ref["c"], bd["c"], sig)
    assert not pmax[:, 2].any() and not pmax[:, 4].any() and not pmin[:, 2].any() and not pmin[:, 4].any()          # a later member of a class never wins


@pytest.mark.parametrize("name", sorted(cv.CASES))
def test_ambiguity_share_of_every_gpu_case(chains, name):
    case = cv.CASES[name]
    ch = chains(case["chain"])
    ref, bd, extra = cv.case_model(ch, cv.inputs(ch, case), probs=())
    share = cv.ambiguity(ref, bd, extra)
    print(f"{name}: {share:.4f} of the (row, draw) pairs are ambiguous")
    assert share <= cv.AMBIGUOUS_MAX, f"{name}: {share:.3f} of the (row, draw) pairs have no certain maximum or minimum"


def test_unused_predictor_is_all_ties(chains):
    ch = chains("unused")
    assert not ch.hit(13, 6).any()
    inp = cv.inputs(ch, cv._case(chain="unused", rows=20, G=4, pool=(5,), var=6))
    ref, bd, extra = cv.case_model(ch, inp)
    assert not ref["r"].any() and not bd["r"].any() and cv.ambiguity(ref, bd, extra) == 0.0
    cmax, pmax, cmin, pmin, _ = cv.counts(ref["c"], bd["c"], extra["sig"])
    want = np.zeros((20, 4), dtype=np.int64)
    want[:, 0] = 5
    assert all(np.array_equal(a, want) for a in (cmax, pmax, cmin, pmin))


def test_chunk_size_rule():
    mib = 1 << 20
    assert cv.chunk_rows(10 ** 6, 400, 20) == 512 * mib // (8 * 400 * 20) // 64 * 64 == 8384
    assert cv.chunk_rows(200, 3, 3, scratch_bytes=8 * 64 * 3 * 3) == 64 and cv.chunk_rows(200, 3, 3, scratch_bytes=1) == 64
    assert cv.chunk_rows(200, 3, 3, scratch_bytes=8 * 127 * 9) == 64 and cv.chunk_rows(200, 3, 3, scratch_bytes=8 * 128 * 9) == 128
    assert cv.chunk_rows(50, 3, 3) == 50 and cv.chunk_rows(10 ** 6, 16384, 64) == 64
    assert cv.chunk_rows(10 ** 9, 1, 1, scratch_bytes=1 << 40) == 512 * mib // 8          # a larger request than the library's own limit: the limit
    from stan4bart_amd.abi import CURVES_SCRATCH_MAX
    assert 8 * 64 * 16384 * 64 <= CURVES_SCRATCH_MAX          # every shape the other limits allow has room for its smallest chunk: that refusal is a second guard


def test_every_refusal_before_any_launch(emul_lib, chains):
    ch = chains("gauss")
    x = ch.x[:7]
    for smp in (ch.live, ch.stored[2]):
        before = ch.live.get_counters()

        def refused(match, vars=0, grid=(0.1, 0.5), **kw):
            with pytest.raises(RuntimeError, match=match):
                smp.predict_curves(x, vars, grid, **kw)
            assert not any(smp.curves_info.values()), smp.curves_info

        refused("predict_curves: nothing asked for", outputs=())
        refused(rf"predictor {ch.P} outside \[0, {ch.P}\)", vars=ch.P)
        refused(rf"predictor -1 outside \[0, {ch.P}\)", vars=-1)
        refused("the two varied predictors must differ", vars=[3, 3], grid=np.zeros((2, 2)))
        refused("between 1 and 64 grid points per call, not 65", grid=np.linspace(0, 1, 65))
        refused("between 1 and 64 grid points per call, not 0", grid=np.zeros(0))
        refused("the grid holds a NaN", grid=(0.1, np.nan))
        refused(r"anchor 2 outside \[-1, 2\)", anchor=2)
        refused(r"anchor -2 outside \[-1, 2\)", anchor=-2)
        refused("between 0 and 16 probs per call, not 17", probs=np.linspace(0, 1, 17))
        refused(r"prob 1.5\d* outside \[0, 1\]", probs=(0.5, 1.5))
        refused(r"prob nan outside \[0, 1\]", probs=(np.nan,))
        refused("quantiles or range_quantiles given, but n_probs = 0", probs=())
        refused("n_probs > 0 needs quantiles", probs=(0.5,), outputs=("mean", "range_quantiles"))
        refused("negative scratch_bytes", outputs=("mean",), scratch_bytes=-1)
        refused("link must be 0", outputs=("mean",), link=2)
        refused("route must be 0", outputs=("mean",), route=3)
        refused("n_peers > 0 needs peer_dense_coef|n_dense > 0 needs peer_dense_coef", outputs=("mean",), peers=[ch.stored[1]], dense=np.ones((7, 1)),
                dense_coef=np.ones((smp.curves_draws(), 1)))
        refused(r"ell_index 5 outside \[-1, 2\)", outputs=("mean",), ell_index=np.full((7, 1), 5), ell_value=np.ones((7, 1)), ell_coef=np.ones((smp.curves_draws(), 2)))
        other = chains("probit").stored[2]
        refused("peer 0 has", outputs=("mean",), peers=[other])
        refused("pooled draws, at most 16384", outputs=("mean",), peers=[ch.stored[13]] * 1300)
        assert np.array_equal(ch.live.get_counters(), before)
        with pytest.raises(ValueError, match="outputs must be among"):
            smp.predict_curves(x, 0, (0.1,), outputs=("median",))
        with pytest.raises(ValueError, match="vars must be one predictor index or two"):
            smp.predict_curves(x, [0, 1, 2], (0.1,))
        with pytest.raises(ValueError, match=r"grid must be \[G\] or \[G x 2\]"):
            smp.predict_curves(x, [0, 1], (0.1, 0.2))


def test_launch_is_refused_on_the_emulated_layer(emul_lib, chains):
    assert hasattr(emul_lib, "emu_predict_curves")
    ch = chains("gauss")
    x = ch.x[:7]
    for smp in (ch.live, ch.stored[5]):
        assert smp.curves_draws() == (13 if smp is ch.live else 5)
        before = ch.live.get_counters()
        with pytest.raises(RuntimeError, match="predict_curves: this device layer has no curve kernels"):
            smp.predict_curves(x, 0, (0.1, 0.5, 0.9), anchor=1, probs=(0.025, 0.975))
        with pytest.raises(RuntimeError, match="no curve kernels"):
            smp.predict_curves(x, [0, 3], np.zeros((4, 2)), outputs=("p_max", "range_mean"), peers=[ch.stored[1], ch.stored[2]])
        assert not any(smp.curves_info.values()) and np.array_equal(ch.live.get_counters(), before)
        with pytest.raises(RuntimeError, match="no partial-dependence kernel"):          # the sibling's refusal is what it was
            smp.partial_dependence(x, 0, (0.1, 0.5))


def test_oracle_library_has_no_entry_and_the_header_has_it(oracle_lib):
    from stan4bart_amd.abi import Sampler
    assert not hasattr(oracle_lib, "orc_predict_curves")
    s = Sampler.__new__(Sampler)
    s._lib, s._pfx = oracle_lib, "orc_"
    with pytest.raises(RuntimeError, match="no predict_curves"):
        Sampler.predict_curves(s, np.zeros((2, 3)), 0, (0.5,))
    header = open(os.path.join(ROOT, "include", "stan4bart_amd.h")).read()
    assert re.search(r"int S4B_FN\(predict_curves\)\(s4b_sampler\* s, const s4b_curves_in\* in, s4b_curves_out\* out\);", header)
    for said in ("THE ORDER OF THE ADDITIONS per (row, grid point, draw) is fixed", "c = range_k * (s_g - s_a)", "LOWEST grid index that attains",
                 "C = scratch / (8 S n_grid) rounded down to a multiple of 64", "S4B_CURVES_SCRATCH_MAX", "quantiles[(j * n_test + i) * n_grid + g]"):
        assert said in header, said


def test_fit_method_checks_its_arguments():
    import summary_cases as sc
    fit, _, _ = sc.fake_fit(0)
    with pytest.raises(ValueError, match="requires 'bart_args' to contain 'keepTrees'"):
        fit.predict_curves(0, np.zeros((3, 2)))
    fit.samplers = [object()]
    xb = np.random.default_rng(0).normal(size=(30, 3))
    with pytest.raises(ValueError, match="'var' must be one column index"):
        fit.predict_curves(3, xb)
    with pytest.raises(ValueError, match="at most 64 per call"):
        fit.predict_curves(0, xb, grid=np.linspace(0, 1, 65))
    with pytest.raises(ValueError, match="'anchor' must be None or a grid index"):
        fit.predict_curves(0, xb, grid=[0.1, 0.2], anchor=2)
    with pytest.raises(ValueError, match="does not form 'ppd'"):
        fit.predict_curves(0, xb, type="ppd")
    with pytest.raises(ValueError, match="grid holds a NaN"):
        fit.predict_curves(0, xb, grid=[0.1, np.nan])
