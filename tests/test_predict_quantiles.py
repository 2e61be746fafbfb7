"""s4b_predict_quantiles without a GPU: the model of tests/quantile_cases.py against np.quantile, the refusals and the pooled tables of
Stan4bartFit.predict_quantiles over stand-in samplers, and the entry on the emulated device layer (no such kernels there: refused with its message).
The kernels are tested in tests/test_gpu_predict_quantiles.py."""
import numpy as np
import pytest

import pd_cases as pc
import quantile_cases as qc
import summary_cases as sc
from conftest import friedman_case

PROBS = (0.0, 1.0, 0.5, 0.025, 0.975, 0.25, 0.75, 0.5, 1.0 / 3.0, 0.999)          # the ends, the median, duplicates, integer and fractional h


@pytest.mark.parametrize("S", [1, 2, 5, 13, 18, 65])
def test_model_matches_numpy_quantile(S):
    g = np.random.default_rng(S)
    v = g.normal(size=(37, S)) * 10.0 ** g.integers(-3, 4, size=(37, 1))
    v[3] = v[3, 0]                                    # a row of ties
    if S > 2:
        v[4, :2] = (-0.0, 0.0)
    got = qc.type7(v, PROBS).astype(np.float64)
    want = np.quantile(v, PROBS, axis=1, method="linear")
    assert got.shape == want.shape == (len(PROBS), 37)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0.0)
    assert np.array_equal(got[0], v.min(axis=1)) and np.array_equal(got[1], v.max(axis=1)) and np.array_equal(got[2], got[7])
    if S % 2:
        assert np.array_equal(got[2], np.sort(v, axis=1)[:, S // 2])          # an integer h returns the order statistic unchanged
    bd = qc.bound(v, np.zeros_like(v), len(PROBS))
    assert bd.shape == got.shape and np.all(bd > 0)
    assert qc.bound_ratio(want, got, bd) <= qc.BOUND_FACTOR          # numpy's own arithmetic lies inside the bound of exact values


def test_model_pools_in_order_with_each_sampler_s_tables():
    rows, q = 9, 7
    g = np.random.default_rng(0)
    lin = sc.linear_parts(rows, 5, 2, 2, q=q)
    parts = [dict(bart=g.normal(size=(rows, s)), dense_coef=g.normal(size=(s, 2)), ell_coef=g.normal(size=(s, q))) for s in (5, 13)]
    shared = dict(dense=lin["dense"], ell_index=lin["ell_index"], ell_value=lin["ell_value"])
    ref, bd, v, bv = qc.model(parts, PROBS, offset=np.ones(rows), **shared)
    assert v.shape == bv.shape == (rows, 18) and ref.shape == bd.shape == (len(PROBS), rows)
    one, _ = sc.model(parts[1]["bart"], np.ones(rows), lin["dense"], parts[1]["dense_coef"], lin["ell_index"], lin["ell_value"], parts[1]["ell_coef"])
    assert np.array_equal(v[:, 5:], one["v"])
    np.testing.assert_allclose(ref, np.quantile(v, PROBS, axis=1), rtol=1e-12)
    swapped, *_ = qc.model(parts[::-1], PROBS, offset=np.ones(rows), **shared)
    assert np.array_equal(swapped, ref)          # a quantile does not see the order of the pool
    ref1, bd1, v1, _ = qc.model(parts, PROBS, link=1, **shared)
    assert np.all((v1 >= 0) & (v1 <= 1)) and np.all(bd1 >= sc.ERFC_C * sc.U)


@pytest.fixture(scope="module")
def emul_chain(emul_lib):
    args, _ = friedman_case(n=100, T=5, warmup=3, iter=6, ranef=False)
    args.keep_trees = True
    c = pc.Chain(emul_lib, "emu_", args, steps=(1, 2), rows=60)
    yield c
    c.close()


def test_entry_is_refused_on_the_emulated_layer(emul_lib, emul_chain):
    assert hasattr(emul_lib, "emu_predict_quantiles")
    x = emul_chain.x[:7]
    for smp in (emul_chain.live, emul_chain.stored[3]):
        before = emul_chain.live.get_counters()
        with pytest.raises(RuntimeError, match="no quantile kernels"):
            smp.predict_quantiles(x, [0.025, 0.975])
        with pytest.raises(RuntimeError, match="no quantile kernels"):
            smp.predict_quantiles(x, [0.5], peers=[emul_chain.stored[1]])
        assert smp.quantile_info["launches"] == 0 and not any(smp.quantile_info.values()) and np.array_equal(emul_chain.live.get_counters(), before)
        with pytest.raises(ValueError, match="probs must be a vector"):
            smp.predict_quantiles(x, [[0.5, 0.6]])
        with pytest.raises(ValueError, match="one table per peer"):
            smp.predict_quantiles(x, [0.5], peers=[emul_chain.stored[1]], dense=np.ones((7, 2)), dense_coef=np.ones((3, 2)), peer_dense_coef=[])
        with pytest.raises(ValueError, match=r"peer_dense_coef\[0\] must be \[1 x 2\]"):
            smp.predict_quantiles(x, [0.5], peers=[emul_chain.stored[1]], dense=np.ones((7, 2)), dense_coef=np.ones((3, 2)), peer_dense_coef=[np.ones((3, 2))])


def test_oracle_library_has_no_entry(oracle_lib):
    from stan4bart_amd.abi import Sampler
    s = Sampler.__new__(Sampler)
    s._lib, s._pfx = oracle_lib, "orc_"
    with pytest.raises(RuntimeError, match="no predict_quantiles"):
        Sampler.predict_quantiles(s, np.zeros((2, 3)), [0.5])


class _Recorder:
    """A stand-in sampler: records the call and answers with the probs repeated over the rows."""

    def __init__(self):
        self.calls = []

    def predict_quantiles(self, x, probs, **kw):
        self.calls.append(dict(x=x, probs=np.array(probs), **kw))
        return dict(quantiles=np.repeat(np.asarray(probs)[:, None], len(x), axis=1), draws=15, info={})


class _NoSampler:
    def predict_quantiles(self, *a, **k):
        raise AssertionError("the ABI was called although the arguments had to be refused")


def test_python_refusals():
    fit, _, _ = sc.fake_fit(0, samplers=[_NoSampler(), _NoSampler()])
    x = np.zeros((40, 3))
    with pytest.raises(ValueError, match="predict_quantiles does not form 'ppd'"):
        fit.predict_quantiles(x, type="ppd")
    for t in ("indiv.fixef", "indiv.ranef"):
        with pytest.raises(ValueError, match="indiv.fixef and indiv.ranef need no trees: use predict"):
            fit.predict_quantiles(x, type=t)
    with pytest.raises(ValueError, match="predict_quantiles needs x_bart"):
        fit.predict_quantiles()
    for bad in ((-0.1, 0.5), (0.5, 1.5), (np.nan,), (), ((0.1, 0.2),)):
        with pytest.raises(ValueError, match=r"'probs' must be a vector of values in \[0, 1\]"):
            fit.predict_quantiles(x, probs=bad)
    bare, _, _ = sc.fake_fit(0)
    with pytest.raises(ValueError, match="predict_quantiles requires 'bart_args' to contain 'keepTrees'"):
        bare.predict_quantiles(x)


def test_one_pooled_call_with_the_per_chain_tables_of_summary_linear():
    a, b, c = _Recorder(), _NoSampler(), _NoSampler()          # the first sampler takes the call, the others travel as its peers
    fit, new_terms, q = sc.fake_fit(0, n_chain=3, samplers=[a, b, c])
    g = np.random.default_rng(4)
    x, X, off = g.normal(size=(40, 3)), g.normal(size=(40, 2)), g.normal(size=40)
    out = fit.predict_quantiles(x, X=X, groups=new_terms, offset=off, seed=5)
    assert np.array_equal(out["probs"], (0.025, 0.5, 0.975)) and out["quantiles"].shape == (3, 40) and out["draws"] == 15
    assert len(a.calls) == 1
    call = a.calls[0]
    linear = fit._summary_linear("ev", X, new_terms, off, True, np.random.default_rng(5))          # the same seed: the same draws of unseen levels
    want = [linear(ch) for ch in range(3)]
    assert want[0]["ell_index"].max() >= q, "no unseen level reached the table"
    assert call["peers"] == [b, c] and np.array_equal(call["x"], x) and np.array_equal(call["probs"], (0.025, 0.5, 0.975))
    for key in ("offset", "dense", "dense_coef", "ell_index", "ell_value", "ell_coef"):
        assert np.array_equal(call[key], want[0][key]), key
    assert call["link"] == 0 and len(call["peer_dense_coef"]) == len(call["peer_ell_coef"]) == 2
    for ch in (1, 2):
        assert np.array_equal(call["peer_dense_coef"][ch - 1], want[ch]["dense_coef"]) and np.array_equal(call["peer_ell_coef"][ch - 1], want[ch]["ell_coef"])
        assert not np.array_equal(want[ch]["ell_coef"], want[0]["ell_coef"])
    ix, val, coef = fit._ell_random(new_terms, True, np.random.default_rng(5))
    assert np.array_equal(call["peer_ell_coef"][1], coef[2]) and np.array_equal(call["ell_index"], ix)
    # the trees alone: no table travels, link 0 whatever the family; a binomial fit's expected value goes through Phi
    a.calls.clear()
    fit.predict_quantiles(x, X=X, groups=new_terms, offset=off, type="indiv.bart", probs=[0.5])
    call = a.calls[0]
    assert call["dense"] is None and call["ell_index"] is None and call["offset"] is None and call["peer_dense_coef"] is None and call["peer_ell_coef"] is None
    a2 = _Recorder()
    fit2, new2, _ = sc.fake_fit(0, family="binomial", samplers=[a2])
    fit2.predict_quantiles(x, groups=new2)
    assert a2.calls[0]["link"] == 1 and a2.calls[0]["peers"] == [] and a2.calls[0]["peer_ell_coef"] == [] and a2.calls[0]["peer_dense_coef"] is None
