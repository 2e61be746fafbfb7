"""s4b_predict_spread without a GPU (tests/spread_cases.py: the model, the bounds, the thresholds): the model against a brute-force numpy loop over the
emulated layer's predict_bart — a slab without weight, T = 0, t = +-inf among them —, the stated order of the additions carried out in double against
the model within the bounds, the binding's argument handling on a fake library call, the refusals and the views of the Python methods, bayes_R2's
arithmetic on a hand-made draws matrix, the refusal on the emulated device layer, the absence from the oracle library and the presence in the header.

test_model_against_brute_force and test_stated_order_lies_within_the_bounds guard the MODEL of tests/spread_cases.py, which the device tests are
measured against, not the product: they use spread_cases and the emulated predict_bart alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pd_cases as pc
import spread_cases as sp
import summary_cases as sc
from conftest import friedman_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS = (0.025, 0.5, 0.975, 0.0, 1.0)


@pytest.fixture(scope="module")
def emul_chain(emul_lib):
    args, _ = friedman_case(n=100, T=5, warmup=3, iter=6, ranef=False)
    args.keep_trees = True
    c = pc.Chain(emul_lib, "emu_", args, steps=(1, 2), rows=300)
    yield c
    c.close()


def _pool(ch):
    return np.concatenate([ch.stored[3].predict_bart(ch.x), ch.stored[1].predict_bart(ch.x)], axis=1)          # [rows x 4]: the pool (3, 1)


def _weights(kind, rows):
    if kind == "none":
        return None
    w = np.random.default_rng(1).uniform(0.0, 2.0, rows)
    if kind == "zero slab":
        w[128:256] = 0.0          # the second slab carries no weight
    if kind == "indicator":
        w = (np.arange(rows) % 3 == 0).astype(np.float64)
    return w


@pytest.mark.parametrize("kind", ["none", "random", "zero slab", "indicator"])
@pytest.mark.parametrize("T", [0, 1, 5])
def test_model_against_brute_force(emul_chain, kind, T):
    x = _pool(emul_chain)
    rows = len(x)
    w = _weights(kind, rows)
    th = sp.thresholds_for(x, T, lo_inf=T >= 5, hi_inf=T >= 5)
    ref, bd = sp.model(x, np.full_like(x, 1e-18), w, th, PROBS)
    assert ref["ambiguous"] == 0 and ref["zero_slabs"] == (1 if kind == "zero slab" else 0)
    assert ref["draws"].shape == (4 + 2 * T, 4) and ref["quantiles"].shape == (len(PROBS), 4 + 2 * T)
    want = sp.brute_force(x, w, th)
    np.testing.assert_allclose(ref["draws"].astype(np.float64), want, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(ref["mean"], want.mean(axis=1), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(ref["quantiles"], np.quantile(want, PROBS, axis=1), rtol=1e-10, atol=1e-12)
    assert ref["weight"] == sp.gc.host_weight(np.ones(rows) if w is None else w)
    if T >= 5:          # t = -inf: every row with weight lies above; t = +inf: none
        D = ref["draws"].astype(np.float64)
        np.testing.assert_allclose(D[4], 1.0, rtol=1e-15)
        np.testing.assert_allclose(D[4 + T], D[0], rtol=1e-13, atol=1e-15)
        assert np.all(D[4 + T - 1] == 0.0) and np.all(D[4 + 2 * T - 1] == 0.0)
    if w is None and T:
        n_above = (x[:, :, None] > th[None, None, :]).sum(axis=0).T
        assert np.array_equal(ref["draws"][4:4 + T].astype(np.float64), n_above / float(rows)) and np.all(bd["draws"][4:4 + T] == 0.0)
    # a threshold ON a value is ambiguous
    r2, _ = sp.model(x, np.full_like(x, 1e-18), w, [float(x[7, 1])])
    assert r2["ambiguous"] >= 1


@pytest.mark.parametrize("kind", ["none", "random", "zero slab", "indicator"])
@pytest.mark.parametrize("rows", [1, 127, 128, 129, 300])
def test_stated_order_lies_within_the_bounds(emul_chain, kind, rows):
    """The header's order of the additions in plain double, with exact inputs (bx = 0), against the long-double model: within the derived bounds;
    the properties the header promises bit for bit hold for it."""
    x = _pool(emul_chain)[:rows] + 40.0          # (a mean far from 0 against the spread: what the shift is for)
    w = _weights(kind, 300)
    w = None if w is None else w[:rows]
    if w is not None and not w.sum() > 0.0:
        w[0] = 1.0
    th = sp.thresholds_for(x, 4, lo_inf=True, hi_inf=True) if rows > 1 else np.array([-np.inf, np.inf])
    ref, bd = sp.model(x, 0.0, w, th)
    D = sp.device_order(x, w, th)
    T = len(th)
    ratios = {k: sp.bound_ratio(D[s], ref["draws"][s], bd["draws"][s]) for k, s in
              (("mean", slice(0, 1)), ("sd", slice(1, 2)), ("minmax", slice(2, 4)), ("share", slice(4, 4 + T)), ("part", slice(4 + T, 4 + 2 * T)))}
    print(f"{rows} rows, weights {kind}: the stated order against the model, ratios to the bound {ratios}")
    assert all(r <= sp.BOUND_FACTOR for r in ratios.values()), ratios
    assert np.all(D[4 + T - 1] == 0.0) and np.all(D[4 + 2 * T - 1] == 0.0)          # t = +inf
    if w is None:
        assert np.all(D[4] == 1.0) and np.array_equal(D[4:4 + T], ref["draws"][4:4 + T].astype(np.float64))
    if rows == 1:
        assert np.array_equal(D[0], x[0]) and np.all(D[1] == 0.0) and np.array_equal(D[2], x[0]) and np.array_equal(D[3], x[0])
    if w is not None:
        assert np.array_equal(sp.device_order(x, 2.0 * w, th), D), "weights times 2 change an output"
    pos, neg = sp.device_order(x, w, [-np.inf]), sp.device_order(-x, w, [-np.inf])          # the arms swapped
    assert np.array_equal(pos[:4], D[:4]), "the moments and the extremes depend on the thresholds"
    assert np.array_equal(neg[0], -pos[0]) and np.array_equal(neg[1], pos[1]) and np.array_equal(neg[2], -pos[3]) and np.array_equal(neg[3], -pos[2])
    assert np.array_equal(neg[5], -pos[5]) and np.array_equal(neg[4], pos[4])


def test_raw_moments_would_not_meet_the_bound():
    """What the shift is for: at a mean of 1e6 and a spread of 1e-3 the raw second moment loses every digit of sd, the stated order keeps it."""
    g = np.random.default_rng(0)
    x = 1e6 + 1e-3 * g.standard_normal((300, 2))
    ref, bd = sp.model(x, 0.0)
    D = sp.device_order(x)
    assert sp.bound_ratio(D[1], ref["draws"][1], bd["draws"][1]) <= sp.BOUND_FACTOR
    raw = np.sqrt(np.maximum(0.0, (x * x).sum(axis=0) / 300 - (x.sum(axis=0) / 300) ** 2))
    assert sp.bound_ratio(raw, ref["draws"][1], bd["draws"][1]) > 100.0
    assert np.all(bd["draws"][1] < 1e-4 * ref["draws"][1].astype(np.float64)), "the bound of sd says nothing at this shape"


class _FakeLib:
    """A library whose predict_spread records what it is handed and answers with fixed numbers: statistic m of draw k is 10 m + k + 1."""

    def __init__(self, draws=3):
        self.draws, self.seen = draws, []
        self.fk_predict_spread = self._call

    def _call(self, handle, arg, out):
        o = out._obj
        o.num_samples = self.draws
        if arg is None:
            return 0
        a = arg._obj
        n, T, S = a.arms.rows.n_test, a.n_thresholds, self.draws
        M = 4 + 2 * T
        self.seen.append(dict(thresholds=np.ctypeslib.as_array(a.thresholds, shape=(T,)).copy() if T else np.zeros(0), n_arms=a.n_arms, bin_index=a.bin_index,
                              n_probs=a.arms.n_probs, scratch=a.arms.scratch_bytes, has=dict(mean=bool(o.mean), m2=bool(o.m2), draws=bool(o.draws), quantiles=bool(o.quantiles)),
                              weights=None if not a.arms.rows.n_weights else np.ctypeslib.as_array(a.arms.rows.weights, shape=(n,)).copy()))
        D = 10.0 * np.arange(M)[:, None] + np.arange(S)[None, :] + 1.0
        if o.draws:
            np.ctypeslib.as_array(o.draws, shape=(M, S))[:] = D
        if o.mean:
            np.ctypeslib.as_array(o.mean, shape=(M,))[:] = D.mean(axis=1)
        if o.m2:
            np.ctypeslib.as_array(o.m2, shape=(M,))[:] = ((D - D.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)
        if a.arms.n_probs:
            pr = np.ctypeslib.as_array(a.arms.probs, shape=(a.arms.n_probs,))
            np.ctypeslib.as_array(o.quantiles, shape=(a.arms.n_probs, M))[:] = np.quantile(D, pr, axis=1)
        o.weight = 7.0
        o.info[5], o.info[6] = S, T
        return 0


def _fake_sampler(lib):
    from stan4bart_amd.abi import Sampler
    s = Sampler.__new__(Sampler)
    s._lib, s._pfx, s._h = lib, "fk_", C.c_void_p(1)
    return s


def test_argument_handling_of_the_binding_on_a_fake_library_call():
    from stan4bart_amd.abi import SPREAD_BIN_INDEX, SPREAD_INFO, SPREAD_SLAB, SPREAD_THRESHOLDS_MAX, Sampler
    assert SPREAD_THRESHOLDS_MAX == sp.THRESHOLDS_MAX == 64 and SPREAD_SLAB == sp.SLAB and len(SPREAD_INFO) == 8 and SPREAD_BIN_INDEX["search"] == 2
    assert Sampler.spread_names(2) == sp.names(2) == ["mean", "sd", "min", "max", "share_above[0]", "share_above[1]", "part_above[0]", "part_above[1]"]
    lib = _FakeLib()
    smp = _fake_sampler(lib)
    x = np.random.default_rng(5).standard_normal((50, 3))
    got = smp.predict_spread(x, thresholds=(-np.inf, 0.5), probs=(0.0, 0.5, 1.0), weights=np.ones(50), scratch_bytes=4096, bin_index="search")
    seen = lib.seen[-1]
    assert np.array_equal(seen["thresholds"], [-np.inf, 0.5]) and seen["n_arms"] == 1 and seen["bin_index"] == 2 and seen["n_probs"] == 3
    assert seen["scratch"] == 4096 and np.array_equal(seen["weights"], np.ones(50)) and seen["has"] == dict(mean=True, m2=True, draws=True, quantiles=True)
    D = 10.0 * np.arange(8)[:, None] + np.arange(3)[None, :] + 1.0
    assert np.array_equal(got["draws"], D) and np.array_equal(got["mean"], D.mean(axis=1)) and np.array_equal(got["m2"], np.full(8, 2.0))
    assert np.array_equal(got["quantiles"], np.quantile(D, (0.0, 0.5, 1.0), axis=1)) and got["names"] == sp.names(2)
    assert got["weight"] == 7.0 and got["draws_pooled"] == 3 and got["info"]["thresholds"] == 2 and np.array_equal(got["thresholds"], [-np.inf, 0.5])
    plain = smp.predict_spread(x, outputs=("mean",))
    assert lib.seen[-1]["has"] == dict(mean=True, m2=False, draws=False, quantiles=False) and lib.seen[-1]["weights"] is None
    assert plain["mean"].shape == (4,) and plain["m2"] is None and plain["draws"] is None and plain["quantiles"] is None and lib.seen[-1]["bin_index"] == 0
    nothing = smp.predict_spread(x, thresholds=0.0, outputs=())          # (still a call, not a query; a scalar threshold is a vector of one)
    assert lib.seen[-1]["has"]["mean"] and nothing["mean"] is None and len(lib.seen[-1]["thresholds"]) == 1
    with pytest.raises(ValueError, match="unknown outputs"):
        smp.predict_spread(x, outputs=("p_above",))
    with pytest.raises(ValueError, match="thresholds must be a vector"):
        smp.predict_spread(x, thresholds=np.zeros((2, 2)))
    with pytest.raises(ValueError, match=r"weights must be \[50\]"):
        smp.predict_spread(x, weights=np.ones((2, 50)))
    with pytest.raises(ValueError, match="bin_index must be one of auto, compare, search"):
        smp.predict_spread(x, bin_index="bisect")


def test_entry_is_refused_on_the_emulated_layer(emul_lib, emul_chain):
    assert hasattr(emul_lib, "emu_predict_spread")
    x = emul_chain.x[:7]
    for smp in (emul_chain.live, emul_chain.stored[3]):
        assert smp.spread_draws() == 3
        before = emul_chain.live.get_counters()
        with pytest.raises(RuntimeError, match="predict_spread: this device layer has no spread kernels"):
            smp.predict_spread(x, thresholds=(0.0,), probs=[0.025, 0.975])
        with pytest.raises(RuntimeError, match="no spread kernels"):
            smp.predict_spread(x, x_test0=x[::-1], n_arms=2, weights=np.ones(7), peers=[emul_chain.stored[1]])
        assert not any(smp.spread_info.values()) and np.array_equal(emul_chain.live.get_counters(), before)
        with pytest.raises(RuntimeError, match="no projection kernels"):          # the sibling's refusal is what it was
            smp.predict_projection(x, np.ones((7, 1)))


def test_oracle_library_has_no_entry_and_the_header_has_it(oracle_lib):
    from stan4bart_amd.abi import Sampler
    assert not hasattr(oracle_lib, "orc_predict_spread")
    s = Sampler.__new__(Sampler)
    s._lib, s._pfx = oracle_lib, "orc_"
    with pytest.raises(RuntimeError, match="no predict_spread"):
        Sampler.predict_spread(s, np.zeros((2, 3)))
    header = open(os.path.join(ROOT, "include", "stan4bart_amd.h")).read()
    assert re.search(r"int S4B_FN\(predict_spread\)\(s4b_sampler\* s, const s4b_spread_in\* in, s4b_spread_out\* out\);", header)
    assert "#define S4B_SPREAD_THRESHOLDS_MAX 64" in header and f"#define S4B_SPREAD_SLAB {sp.SLAB}" in header
    for said in ("THE ORDER OF THE ADDITIONS", "the shift c = the value of the slab's first row", "delta = mean_b - mean_a", "from b = T downward",
                 "A partial with W_s = 0 is skipped", "clamped at 0"):
        assert said in header, said


class _Recorder:
    """A stand-in sampler of 15 draws per chain: records the call and answers with a matrix the views can be checked on."""

    def __init__(self, draws=15):
        self.calls, self.draws = [], draws

    def matrix(self, T, S):
        D = np.zeros((4 + 2 * T, S))
        k = np.arange(S, dtype=np.float64)
        D[0], D[1], D[2], D[3] = 2.0 + k, 0.5 + 0.25 * k, -1.0, 9.0
        for j in range(T):
            D[4 + j] = np.where(k % (j + 2) == 0, 0.0, 0.5)          # some draws without a row above
            D[4 + T + j] = np.where(k % (j + 2) == 0, 0.0, 1.5 + j)
        return D

    def predict_spread(self, **kw):
        self.calls.append(kw)
        T, Q, S = len(kw["thresholds"]), len(kw["probs"]), self.draws * (1 + len(kw["peers"]))
        D = self.matrix(T, S)
        return dict(draws=D, mean=D.mean(axis=1), m2=((D - D.mean(axis=1, keepdims=True)) ** 2).sum(axis=1), quantiles=np.quantile(D, kw["probs"], axis=1) if Q else None,
                    names=sp.names(T), weight=3.5, thresholds=np.asarray(kw["thresholds"]), draws_pooled=S, info={"thresholds": T})


class _NoSampler:
    def predict_spread(self, *a, **k):
        raise AssertionError("the ABI was called although the arguments had to be refused")


def test_python_refusals():
    fit, new_terms, _ = sc.fake_fit(0, samplers=[_NoSampler(), _NoSampler()])
    x = np.zeros((40, 3))
    with pytest.raises(ValueError, match="predict_spread does not form 'ppd'"):
        fit.predict_spread(x, type="ppd")
    with pytest.raises(ValueError, match="indiv.fixef and indiv.ranef need no trees: use predict"):
        fit.predict_spread(x, type="indiv.ranef")
    with pytest.raises(ValueError, match="predict_spread needs x_bart"):
        fit.predict_spread()
    with pytest.raises(ValueError, match="at most 16 values in"):
        fit.predict_spread(x, probs=[1.5])
    with pytest.raises(ValueError, match="'thresholds' must be a vector of at most 64 values, not 65"):
        fit.predict_spread(x, thresholds=np.arange(65.0))
    with pytest.raises(ValueError, match="'thresholds' holds a NaN"):
        fit.predict_spread(x, thresholds=[0.0, np.nan])
    for bad in ([1.0, 0.0], [0.0, 0.0], [np.inf, np.inf]):
        with pytest.raises(ValueError, match="'thresholds' must be strictly ascending"):
            fit.predict_spread(x, thresholds=bad)
    for bad in (np.full(40, -1.0), np.full(40, np.nan), np.full(40, np.inf), np.ones(39)):
        with pytest.raises(ValueError, match="row_weights must be .40. finite non-negative values"):
            fit.predict_spread(x, row_weights=bad)
    with pytest.raises(ValueError, match="row_weights sum to 0"):
        fit.predict_spread(x, row_weights=np.zeros(40))
    with pytest.raises(ValueError, match="'treatment' builds both arms from one row set"):
        fit.predict_spread(x, x_bart0=x, treatment=("x_bart", 0))
    with pytest.raises(ValueError, match="X0 given without X"):
        fit.predict_spread(x, X0=np.zeros((40, 2)))
    none = sc.fake_fit(0)[0]
    with pytest.raises(ValueError, match="predict_spread requires 'bart_args' to contain 'keepTrees' as True"):
        none.predict_spread(x)
    binary = sc.fake_fit(0, family="binomial", samplers=[_NoSampler()])[0]
    with pytest.raises(ValueError, match="bayes_R2 is defined here for a continuous response only"):
        binary.bayes_R2(x)
    with pytest.raises(ValueError, match="bayes_R2 needs x_bart"):
        fit.bayes_R2()
    with pytest.raises(ValueError, match="bayes_R2 needs at least two rows"):
        fit.bayes_R2(x[:1])


def test_views_and_the_pooled_call():
    a = _Recorder()
    fit, new_terms, _ = sc.fake_fit(0, n_chain=3, samplers=[a, _NoSampler(), _NoSampler()])
    g = np.random.default_rng(4)
    rows = 40
    x, X, off = g.normal(size=(rows, 3)), g.normal(size=(rows, 2)), g.normal(size=rows)
    w = g.uniform(0.5, 1.5, rows)
    th = (-0.5, 2.0)
    got = fit.predict_spread(x, X=X, groups=new_terms, offset=off, row_weights=w, thresholds=th, seed=3)
    call = a.calls[-1]
    assert call["n_arms"] == 1 and np.array_equal(call["weights"], w) and call["x_test0"] is None and np.array_equal(call["thresholds"], th)
    assert len(call["peers"]) == 2 and len(call["peer_dense_coef"]) == 2 and call["link"] == 0 and np.array_equal(call["dense"], X - fit.X_means)
    assert set(call["outputs"]) == {"mean", "m2", "draws"}
    S, T = 45, 2
    D = a.matrix(T, S)
    assert got["draws"] == S and got["names"] == sp.names(T) and got["weight"] == 3.5 and np.array_equal(got["thresholds"], th) and "matrix" not in got
    assert np.array_equal(got["mean"], D.mean(axis=1)) and np.allclose(got["sd"], D.std(axis=1, ddof=1)) and got["quantiles"].shape == (3, 8)
    assert got["effect_sd"]["mean"] == D[1].mean() and np.array_equal(got["effect_sd"]["quantiles"], np.quantile(D[1], (0.025, 0.5, 0.975)))
    assert np.array_equal(got["share_above"]["mean"], D[4:6].mean(axis=1)) and got["part_above"]["quantiles"].shape == (3, 2)
    # the derived views: NaN in the draws without a row above, so NaN in their summaries here
    assert np.all(np.isnan(got["mean_above"]["mean"])) and np.all(np.isnan(got["gain"]["mean"]))
    full = fit.predict_spread(x, thresholds=th, return_draws=True, probs=())
    assert np.array_equal(full["matrix"], D) and np.array_equal(full["effect_sd"], D[1]) and np.array_equal(full["share_above"], D[4:6])
    none = D[4:6] == 0.0
    assert np.array_equal(np.isnan(full["mean_above"]), none) and np.array_equal(np.isnan(full["gain"]), none)
    assert np.array_equal(full["mean_above"][~none], (D[6:8] / np.where(none, 1.0, D[4:6]))[~none])
    assert np.array_equal(full["gain"][~none], (D[6:8] - np.array(th)[:, None] * D[4:6])[~none])
    assert full["quantiles"].shape == (0, 8) and a.calls[-1]["weights"] is None
    # no thresholds: four statistics, empty views
    bare = fit.predict_spread(x, thresholds=(), return_draws=True)
    assert bare["names"] == ["mean", "sd", "min", "max"] and bare["share_above"].shape == (0, S) and bare["gain"].shape == (0, S)
    # any arm-0 argument, or treatment=, makes it the contrast
    fit.predict_spread(x, X=X, groups=new_terms, treatment=("X", 1))
    call = a.calls[-1]
    assert call["n_arms"] == 2 and call["dense0"] is not None and call["x_test0"] is None and np.array_equal(call["thresholds"], [0.0])
    assert np.all(call["dense"][:, 1] == 1.0 - fit.X_means[1]) and np.all(call["dense0"][:, 1] == 0.0 - fit.X_means[1])
    fit.predict_spread(x, x_bart0=x + 1.0, type="indiv.bart")
    assert a.calls[-1]["n_arms"] == 2 and np.array_equal(a.calls[-1]["x_test0"], x + 1.0) and a.calls[-1].get("dense") is None


def test_bayes_r2_arithmetic_on_a_hand_made_matrix():
    """R2_k = v_k / (v_k + sigma_k^2), v_k = R's var of the fitted values over the rows, sigma lined up with the pooled order: chain after chain."""
    from stan4bart_amd.generics import Stan4bartFit
    a = _Recorder(draws=5)
    fit, new_terms, _ = sc.fake_fit(0, n_iter=5, n_chain=3, samplers=[a, _NoSampler(), _NoSampler()])
    rows = 40
    x = np.random.default_rng(2).normal(size=(rows, 3))
    got = fit.bayes_R2(x, probs=(0.1, 0.9))
    call = a.calls[-1]
    assert call["n_arms"] == 1 and len(call["thresholds"]) == 0 and len(call["probs"]) == 0 and call["link"] == 0 and call["weights"] is None
    S = 15
    sd = a.matrix(0, S)[1]
    sig = fit.stan[fit.par_names.index("aux.1")]          # [iter, chain]
    sigma = np.concatenate([sig[:, c] for c in range(3)])
    v = sd ** 2 * rows / (rows - 1)
    want = v / (v + sigma ** 2)
    np.testing.assert_allclose(got["r2"], want, rtol=1e-14)
    assert got["mean"] == got["r2"].mean() and got["median"] == np.median(got["r2"])
    assert np.array_equal(got["quantiles"], np.quantile(got["r2"], (0.1, 0.9))) and np.all((want > 0.0) & (want < 1.0))
    # by hand: a fit of variance 4 across 5 rows (population sd sqrt(3.2)) against sigma 2 is one half
    assert Stan4bartFit.r2_from_spread([np.sqrt(3.2)], [2.0], 5)[0] == pytest.approx(0.5, abs=1e-15)
    fitted = np.random.default_rng(3).normal(size=(7, 4))
    r2 = Stan4bartFit.r2_from_spread(fitted.std(axis=0), np.ones(4), 7)
    np.testing.assert_allclose(r2, fitted.var(axis=0, ddof=1) / (fitted.var(axis=0, ddof=1) + 1.0), rtol=1e-14)
    with pytest.raises(ValueError, match="4 draws of the spread, but 3 of sigma"):
        Stan4bartFit.r2_from_spread(np.ones(4), np.ones(3), 7)
