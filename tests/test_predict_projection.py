"""s4b_predict_projection without a GPU (tests/projection_cases.py: the model, the bounds, the designs): the model against np.linalg.lstsq over the
emulated layer's predict_bart, the binding's power-of-two column scaling and its inverse on a fake library call, the refusals, the centring and the
names of the Python method, the refusal on the emulated device layer, the absence from the oracle library and the presence in the header.

test_model_against_lstsq guards the MODEL of tests/projection_cases.py, which the device tests are measured against, not the product: it uses
projection_cases and the emulated predict_bart alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pd_cases as pc
import projection_cases as pj
import summary_cases as sc
from conftest import friedman_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS = (0.025, 0.5, 0.975, 0.0, 1.0)


@pytest.fixture(scope="module")
def emul_chain(emul_lib):
    args, _ = friedman_case(n=100, T=5, warmup=3, iter=6, ranef=False)
    args.keep_trees = True
    c = pc.Chain(emul_lib, "emu_", args, steps=(1, 2), rows=200)
    yield c
    c.close()


@pytest.mark.parametrize("weighted", [False, True])
def test_model_against_lstsq(emul_chain, weighted):
    ch, rows, K = emul_chain, 200, 5
    x = np.concatenate([ch.stored[3].predict_bart(ch.x), ch.stored[1].predict_bart(ch.x)], axis=1)          # [rows x 4]: the pool (3, 1)
    A = pj.design_matrix(rows, K, seed=1)
    w = np.random.default_rng(1).uniform(0.0, 2.0, rows) if weighted else None
    if weighted:
        w[128:] = 0.0          # a part of the rows without weight
    ref, bd = pj.model(x, np.zeros_like(x), A, w, PROBS)
    assert ref["deficient"] == 0
    ww = np.ones(rows) if w is None else w
    # form 1: ordinary least squares of sqrt(w) x on sqrt(w) A
    r = np.sqrt(ww)[:, None]
    beta, *_ = np.linalg.lstsq(r * A, r * x, rcond=None)
    np.testing.assert_allclose(ref["coef"].astype(np.float64), beta, rtol=1e-10, atol=1e-12)
    # form 2: the normal equations and the weighted variance of the residuals
    beta2 = np.linalg.solve(A.T @ (ww[:, None] * A), A.T @ (ww[:, None] * x))
    np.testing.assert_allclose(ref["coef"].astype(np.float64), beta2, rtol=1e-10, atol=1e-12)
    res = x - A @ beta
    mean = (ww @ x) / ww.sum()
    want = 1.0 - (ww @ (res * res)) / (ww @ ((x - mean) ** 2))
    np.testing.assert_allclose(ref["r2"].astype(np.float64), want, rtol=1e-8, atol=1e-10)
    M = np.vstack([beta, want[None, :]])
    np.testing.assert_allclose(ref["mean"], M.mean(axis=1), rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(ref["quantiles"], np.quantile(M, PROBS, axis=1), rtol=1e-8, atol=1e-10)
    assert ref["weight"] == pj.gc.host_weight(ww)
    # with exact inputs the moments' bound is the reduction's own
    n = rows
    adds = min(n, pj.SLAB) + -(-n // pj.SLAB) + 1
    np.testing.assert_allclose(bd["coef"].shape, (K, 4))
    np.testing.assert_allclose(ref["moments"]["bs"], adds * pj.U * (ww @ np.abs(x)), rtol=1e-12)
    cond, worst = pj.check_inputs(ref, bd, "the test design")
    assert cond >= 1.0 and worst > 0.0
    # thresholds: midway between two adjacent values nothing is ambiguous, on a value that value is
    M_ref = np.vstack([ref["coef"].astype(np.float64), ref["r2"].astype(np.float64)[None, :]])
    t = pj.gc.midway(M_ref)
    r2, _ = pj.model(x, np.full_like(x, 1e-18), A, w, threshold=t)
    assert r2["ambiguous"] == 0 and np.array_equal(r2["p_above"], (M_ref > t).mean(axis=1))
    r3, _ = pj.model(x, np.full_like(x, 1e-18), A, w, threshold=float(M_ref[1, 0]))
    assert r3["ambiguous"] >= 1


def test_model_flags_what_has_no_answer():
    g = np.random.default_rng(3)
    x, A = g.standard_normal((40, 3)), pj.design_matrix(40, 4)
    dup = np.column_stack([A, A[:, 2]])
    ref, _ = pj.model(x, 0.0, dup, probs=PROBS, threshold=0.0)
    assert ref["deficient"] == 1 and np.all(np.isnan(ref["coef"])) and np.all(np.isnan(ref["p_above"])) and ref["quantiles"].shape == (5, 6)
    assert pj.model(x, 0.0, A, np.zeros(40))[0]["deficient"] == 2
    assert pj.model(x[:0], 0.0, A[:0])[0]["deficient"] == 3
    # a constant series: tss == 0 up to rounding is NaN only where it is exactly 0
    ones = np.ones((40, 1))
    r, _ = pj.model(ones, 0.0, A[:, :1])
    assert r["deficient"] == 0 and r["coef"][0, 0] == 1.0 and np.isnan(r["r2"][0])
    L, bad = pj.cholesky(np.array([[4.0, 2.0], [2.0, 1.0]]))
    assert bad and L[0, 0] == 2.0
    assert pj.padded_columns(8) == 8 and pj.padded_columns(9) == 16 and pj.padded_columns(17) == 32


class _FakeLib:
    """A library whose predict_projection records the design it is handed and answers with fixed numbers: coefficient j of draw k is 10 j + k + 1."""

    def __init__(self, draws=3):
        self.draws, self.seen = draws, []
        self.fk_predict_projection = self._call

    def _call(self, handle, arg, out):
        o = out._obj
        o.num_samples = self.draws
        if arg is None:
            return 0
        a = arg._obj
        n, K, S = a.arms.rows.n_test, a.n_columns, self.draws
        self.seen.append(dict(design=np.ctypeslib.as_array(a.design, shape=(n, K)).copy(), threshold=a.threshold, has_threshold=a.has_threshold, tol=a.tol,
                              n_arms=a.n_arms, weights=None if not a.arms.rows.n_weights else np.ctypeslib.as_array(a.arms.rows.weights, shape=(n,)).copy()))
        coef = np.ctypeslib.as_array(o.coef, shape=(K, S))
        coef[:] = 10.0 * np.arange(K)[:, None] + np.arange(S)[None, :] + 1.0
        np.ctypeslib.as_array(o.r2, shape=(S,))[:] = 0.5
        M = np.vstack([coef, np.full((1, S), 0.5)])
        np.ctypeslib.as_array(o.mean, shape=(K + 1,))[:] = M.mean(axis=1)
        np.ctypeslib.as_array(o.m2, shape=(K + 1,))[:] = ((M - M.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)
        if a.arms.n_probs:
            pr = np.ctypeslib.as_array(a.arms.probs, shape=(a.arms.n_probs,))
            np.ctypeslib.as_array(o.quantiles, shape=(a.arms.n_probs, K + 1))[:] = np.quantile(M, pr, axis=1)
        if a.has_threshold:
            np.ctypeslib.as_array(o.p_above, shape=(K + 1,))[:] = (M > a.threshold).mean(axis=1)
        o.weight = 7.0
        o.info[5], o.info[7] = S, K
        return 0


def _fake_sampler(lib):
    from stan4bart_amd.abi import Sampler
    s = Sampler.__new__(Sampler)
    s._lib, s._pfx, s._h = lib, "fk_", C.c_void_p(1)
    return s


def test_column_scaling_of_the_binding_on_a_fake_library_call():
    from stan4bart_amd.abi import PROJECTION_COLUMNS_MAX, PROJECTION_INFO, PROJECTION_SLAB, Sampler
    assert PROJECTION_COLUMNS_MAX == pj.COLUMNS_MAX == 32 and PROJECTION_SLAB == pj.SLAB and len(PROJECTION_INFO) == 8
    g = np.random.default_rng(5)
    A = g.standard_normal((50, 4)) * np.array([1.0, 1000.0, 3e-5, 0.7])
    A[:, 0] = 1.0
    scale = Sampler.column_scales(A)
    rms = np.sqrt((A * A).mean(axis=0))
    assert np.all(np.frexp(scale)[0] == 0.5), "a scale is not a power of two"
    assert np.all(scale * rms > 2.0 ** -0.5 - 1e-12) and np.all(scale * rms < 2.0 ** 0.5 + 1e-12) and scale[0] == 1.0
    assert np.array_equal(Sampler.column_scales(np.zeros((5, 2))), [1.0, 1.0])
    lib = _FakeLib()
    smp = _fake_sampler(lib)
    x = g.standard_normal((50, 3))
    got = smp.predict_projection(x, A, probs=(0.0, 0.5, 1.0), threshold=12.0, weights=np.ones(50), tol=1e-8)
    seen = lib.seen[-1]
    assert np.array_equal(seen["design"], A * scale) and np.array_equal(seen["design"] / scale, A), "the scaling is not exact"
    assert seen["threshold"] == 12.0 and seen["has_threshold"] == 1 and seen["tol"] == 1e-8 and seen["n_arms"] == 1 and np.array_equal(seen["weights"], np.ones(50))
    raw = 10.0 * np.arange(4)[:, None] + np.arange(3)[None, :] + 1.0
    assert np.array_equal(got["coef"], raw * scale[:, None]) and np.array_equal(got["scale"], scale)
    assert np.array_equal(got["mean"][:4], raw.mean(axis=1) * scale) and got["mean"][4] == 0.5
    assert np.array_equal(got["m2"][:4], 2.0 * scale * scale) and got["m2"][4] == 0.0
    assert np.array_equal(got["quantiles"][:, :4], np.quantile(raw, (0.0, 0.5, 1.0), axis=1) * scale) and np.all(got["quantiles"][:, 4] == 0.5)
    assert np.array_equal(got["p_above"][:4], (got["coef"] > 12.0).mean(axis=1)) and got["p_above"][4] == 0.0
    assert got["weight"] == 7.0 and got["draws_pooled"] == 3 and got["deficient"] == 0 and got["info"]["columns"] == 4
    plain = smp.predict_projection(x, A, scale_columns=False)
    assert np.array_equal(lib.seen[-1]["design"], A) and np.array_equal(plain["coef"], raw) and plain["p_above"] is None and plain["quantiles"] is None
    assert lib.seen[-1]["has_threshold"] == 0 and lib.seen[-1]["weights"] is None
    with pytest.raises(ValueError, match=r"design must be \[50 x K\]"):
        smp.predict_projection(x, A[:7])
    with pytest.raises(ValueError, match=r"weights must be \[50\]"):
        smp.predict_projection(x, A, weights=np.ones((2, 50)))


def test_entry_is_refused_on_the_emulated_layer(emul_lib, emul_chain):
    assert hasattr(emul_lib, "emu_predict_projection")
    x = emul_chain.x[:7]
    A = pj.design_matrix(7, 2)
    for smp in (emul_chain.live, emul_chain.stored[3]):
        assert smp.projection_draws() == 3
        before = emul_chain.live.get_counters()
        with pytest.raises(RuntimeError, match="predict_projection: this device layer has no projection kernels"):
            smp.predict_projection(x, A, probs=[0.025, 0.975])
        with pytest.raises(RuntimeError, match="no projection kernels"):
            smp.predict_projection(x, A, x_test0=x[::-1], n_arms=2, weights=np.ones(7), peers=[emul_chain.stored[1]], threshold=0.0)
        assert not any(smp.projection_info.values()) and np.array_equal(emul_chain.live.get_counters(), before)
        with pytest.raises(RuntimeError, match="no level kernels"):          # the sibling's refusal is what it was
            smp.predict_groups(x, np.zeros(7, dtype=np.int64), 1)


def test_oracle_library_has_no_entry_and_the_header_has_it(oracle_lib):
    from stan4bart_amd.abi import Sampler
    assert not hasattr(oracle_lib, "orc_predict_projection")
    s = Sampler.__new__(Sampler)
    s._lib, s._pfx = oracle_lib, "orc_"
    with pytest.raises(RuntimeError, match="no predict_projection"):
        Sampler.predict_projection(s, np.zeros((2, 3)), np.ones((2, 1)))
    header = open(os.path.join(ROOT, "include", "stan4bart_amd.h")).read()
    assert re.search(r"int S4B_FN\(predict_projection\)\(s4b_sampler\* s, const s4b_projection_in\* in, s4b_projection_out\* out\);", header)
    assert "#define S4B_PROJECTION_COLUMNS_MAX 32" in header and f"#define S4B_PROJECTION_SLAB {pj.SLAB}" in header
    assert "ACTS ON THE NORMAL EQUATIONS" in header and "ORDER OF THE ADDITIONS" in header


class _Recorder:
    """A stand-in sampler of 15 draws: records the call and answers with the column numbers."""

    def __init__(self, draws=15):
        self.calls, self.draws = [], draws

    def predict_projection(self, **kw):
        self.calls.append(kw)
        K, Q, S = kw["design"].shape[1], len(kw["probs"]), self.draws * (1 + len(kw["peers"]))
        base = np.arange(K + 1, dtype=np.float64)
        return dict(coef=np.tile(base[:K, None], (1, S)), r2=np.full(S, 0.25), mean=base.copy(), m2=np.full(K + 1, 11.0), quantiles=np.tile(base, (Q, 1)) if Q else None,
                    p_above=None if kw["threshold"] is None else base / 100.0, weight=3.5, scale=np.ones(K), deficient=0, draws_pooled=S, info={"columns": K})


class _NoSampler:
    def predict_projection(self, *a, **k):
        raise AssertionError("the ABI was called although the arguments had to be refused")


def test_python_refusals():
    fit, new_terms, _ = sc.fake_fit(0, samplers=[_NoSampler(), _NoSampler()])
    x, A = np.zeros((40, 3)), np.random.default_rng(0).standard_normal((40, 2))
    with pytest.raises(ValueError, match="predict_projection does not form 'ppd'"):
        fit.predict_projection(A, x, type="ppd")
    with pytest.raises(ValueError, match="indiv.fixef and indiv.ranef need no trees: use predict"):
        fit.predict_projection(A, x, type="indiv.ranef")
    with pytest.raises(ValueError, match="predict_projection needs x_bart"):
        fit.predict_projection(A)
    with pytest.raises(ValueError, match="at most 16 values in"):
        fit.predict_projection(A, x, probs=[1.5])
    with pytest.raises(ValueError, match="'threshold' is a NaN"):
        fit.predict_projection(A, x, threshold=np.nan)
    with pytest.raises(ValueError, match=r"'tol' must lie in \[0, 1\)"):
        fit.predict_projection(A, x, tol=1.0)
    with pytest.raises(ValueError, match=r"'design' must hold one row per row of x_bart \(40\)"):
        fit.predict_projection(A[:7], x)
    with pytest.raises(ValueError, match="'design' holds a value that is not finite"):
        fit.predict_projection(np.where(np.arange(80).reshape(40, 2) == 5, np.inf, A), x)
    with pytest.raises(ValueError, match="between 1 and 32 design columns, the intercept included, not 33"):
        fit.predict_projection(np.zeros((40, 32)), x)
    with pytest.raises(ValueError, match="between 1 and 32 design columns, the intercept included, not 0"):
        fit.predict_projection(np.zeros((40, 0)), x, intercept=False)
    with pytest.raises(ValueError, match="3 design columns, the intercept included, but only 2 rows"):
        fit.predict_projection(A[:2], x[:2])
    with pytest.raises(ValueError, match="'names' must name the 2 columns"):
        fit.predict_projection(A, x, names=["age"])
    for bad in (np.full(40, -1.0), np.full(40, np.nan), np.full(40, np.inf), np.ones(39)):
        with pytest.raises(ValueError, match="row_weights must be .40. finite non-negative values"):
            fit.predict_projection(A, x, row_weights=bad)
    with pytest.raises(ValueError, match="'treatment' builds both arms from one row set"):
        fit.predict_projection(A, x, x_bart0=x, treatment=("x_bart", 0))
    with pytest.raises(ValueError, match="X0 given without X"):
        fit.predict_projection(A, x, X0=np.zeros((40, 2)))
    none = sc.fake_fit(0)[0]
    with pytest.raises(ValueError, match="predict_projection requires 'bart_args' to contain 'keepTrees' as True"):
        none.predict_projection(A, x)


def test_centring_names_and_the_pooled_call():
    a = _Recorder()
    fit, new_terms, _ = sc.fake_fit(0, n_chain=3, samplers=[a, _NoSampler(), _NoSampler()])
    g = np.random.default_rng(4)
    rows = 40
    x, X, off = g.normal(size=(rows, 3)), g.normal(size=(rows, 2)), g.normal(size=rows)
    A = g.normal(size=(rows, 2)) + np.array([5.0, -3.0])
    w = g.uniform(0.5, 1.5, rows)
    got = fit.predict_projection(A, x, X=X, groups=new_terms, offset=off, row_weights=w, names=["age", "score"], seed=3)
    call = a.calls[-1]
    centre = (w @ A) / w.sum()
    assert got["names"] == ["(Intercept)", "age", "score"] and np.array_equal(got["center"], np.r_[0.0, centre])
    assert np.array_equal(call["design"], np.column_stack([np.ones(rows), A - centre])) and np.allclose(w @ call["design"][:, 1:], 0.0, atol=1e-12)
    assert call["n_arms"] == 1 and call["threshold"] == 0.0 and call["tol"] == 1e-10 and np.array_equal(call["weights"], w) and call["x_test0"] is None
    assert len(call["peers"]) == 2 and len(call["peer_dense_coef"]) == 2 and call["link"] == 0 and np.array_equal(call["dense"], X - fit.X_means)
    assert got["draws"] == 45 and got["coef"].shape == (3, 45) and got["r2"].shape == (45,) and got["r2_mean"] == 3.0
    assert np.array_equal(got["mean"], [0.0, 1.0, 2.0]) and np.array_equal(got["sd"], np.sqrt(np.full(3, 11.0) / 44))
    assert got["quantiles"].shape == (3, 3) and np.array_equal(got["r2_quantiles"], [3.0, 3.0, 3.0]) and np.array_equal(got["p_above"], [0.0, 0.01, 0.02])
    assert got["weight"] == 3.5 and got["deficient"] == 0 and np.array_equal(got["probs"], [0.025, 0.5, 0.975])
    # without centring, without an intercept, a single column as a vector, default names
    fit.predict_projection(A, x, center=False)
    assert np.array_equal(a.calls[-1]["design"], np.column_stack([np.ones(rows), A])) and a.calls[-1]["weights"] is None
    plain = fit.predict_projection(A[:, 0], x, intercept=False, threshold=None, probs=())
    assert np.array_equal(a.calls[-1]["design"], A[:, :1]) and plain["names"] == ["x1"] and plain["p_above"] is None and plain["quantiles"].shape == (0, 1)
    assert np.array_equal(plain["center"], [0.0])
    unweighted = fit.predict_projection(A, x)
    assert np.allclose(unweighted["center"][1:], A.mean(axis=0)) and unweighted["names"] == ["(Intercept)", "x1", "x2"]
    # any arm-0 argument, or treatment=, makes it the contrast
    fit.predict_projection(A, x, X=X, groups=new_terms, treatment=("X", 1))
    call = a.calls[-1]
    assert call["n_arms"] == 2 and call["dense0"] is not None and call["x_test0"] is None
    assert np.all(call["dense"][:, 1] == 1.0 - fit.X_means[1]) and np.all(call["dense0"][:, 1] == 0.0 - fit.X_means[1])
    fit.predict_projection(A, x, x_bart0=x + 1.0, type="indiv.bart")
    assert a.calls[-1]["n_arms"] == 2 and np.array_equal(a.calls[-1]["x_test0"], x + 1.0) and a.calls[-1].get("dense") is None
