"""s4b_predict_summary without a GPU: the model of tests/summary_cases.py against itself, the ELL builder and the chain pooling of
Stan4bartFit.predict_summary against numpy, the refusals of the Python layer, and the entry on the emulated device layer (which has no summary
kernel: the entry exists and is refused with its message).  The kernels are tested in tests/test_gpu_predict_summary.py."""
import numpy as np
import pytest

import summary_cases as sc
from conftest import friedman_case, make_sampler


def test_welford_matches_numpy_variance():
    g = np.random.default_rng(1)
    for S in (1, 2, 5, 64):
        v = g.normal(size=(7, S)) * 10.0 ** g.integers(-3, 4, size=(7, 1)) + 100.0
        mean, m2 = sc.welford(v)
        np.testing.assert_allclose(mean, v.mean(axis=1), rtol=1e-14)
        np.testing.assert_allclose(m2, S * np.var(v, axis=1), rtol=1e-9, atol=1e-18)
        ref, _ = sc.model(v)
        np.testing.assert_allclose(ref["mean"], mean, rtol=1e-14)
        np.testing.assert_allclose(ref["m2"], m2, rtol=1e-9, atol=1e-18)
    mean, m2 = sc.welford(np.array([[3.25]]))
    assert mean[0] == 3.25 and m2[0] == 0.0                            # one draw: its value, exactly, and exactly no spread


def test_chan_pooling_matches_the_pooled_matrix():
    from stan4bart_amd.generics import Stan4bartFit
    g = np.random.default_rng(2)
    chains = [g.normal(loc=c, size=(9, S)) for c, S in enumerate((5, 1, 8, 3))]
    parts = [(v.shape[1],) + sc.welford(v) for v in chains]
    pooled = np.concatenate(chains, axis=1)
    for pool in (sc.chan_pool, Stan4bartFit._pool_chains):
        n, mean, m2 = pool(parts)
        assert n == pooled.shape[1]
        np.testing.assert_allclose(mean, pooled.mean(axis=1), rtol=1e-13)
        np.testing.assert_allclose(m2 / (n - 1), np.var(pooled, axis=1, ddof=1), rtol=1e-12)


def test_model_weighted_averages_and_links():
    g = np.random.default_rng(3)
    rows, S = 50, 6
    bart = g.normal(size=(rows, S))
    parts = sc.linear_parts(rows, S, 3, 3, seed=1)
    w = sc.weight_vectors(rows, 3)
    off = g.normal(size=rows)
    ref, bound = sc.model(bart, off, weights=w, **parts)
    z = bart + off[:, None] + parts["dense"] @ parts["dense_coef"].T
    ix = parts["ell_index"]
    assert (ix == -1).any() and (ix == 0).any() and (ix == 6).any() and {int(n) for n in (ix >= 0).sum(axis=1)} == {0, 1, 2, 3}
    for e in range(3):
        on = ix[:, e] >= 0
        z[on] += parts["ell_value"][on, e][:, None] * parts["ell_coef"][:, ix[on, e]].T
    np.testing.assert_allclose(ref["v"], z, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref["average"], (w @ z).T, rtol=1e-12, atol=1e-14)
    assert np.all(bound["v"] > 0) and np.all(bound["average"] > 0) and bound["v"].max() < 1e-12
    assert w[0].sum() == pytest.approx(1.0) and (w[2] == 0).any() and (w[2] < 0).any()
    ref1, bound1 = sc.model(bart, off, weights=w, link=1, erfc_c=4.0, **parts)
    from stan4bart_amd.generics import _pnorm
    np.testing.assert_allclose(ref1["v"], _pnorm(z), rtol=0, atol=1e-15)
    assert np.all(bound1["v"] >= 4.0 * sc.U)
    exact, b0 = sc.model(bart)                                        # no linear part: z is the BART fit itself, the bound of z is zero
    assert np.array_equal(exact["v"], bart) and not b0["v"].any()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("sample_new", [True, False])
def test_ell_builder_matches_fitted_random(seed, sample_new):
    """The ELL table of the random part reproduces _fitted_random (np.einsum over [p, level, iter, chain]) draw for draw, unseen levels drawn with the
    same generator calls in the same order."""
    fit, new_terms, q = sc.fake_fit(seed)
    want = fit._fitted_random(new_terms, False, False, sample_new, np.random.default_rng(seed + 40))       # [rows, iter, chain]
    ix, val, coef = fit._ell_random(new_terms, sample_new, np.random.default_rng(seed + 40))
    rows = want.shape[0]
    assert ix.dtype == np.int32 and ix.shape == val.shape == (rows, sum(t.p for t in new_terms)) and len(coef) == 2
    unseen = np.column_stack([np.repeat((np.asarray(t.levels) > ft.l)[:, None], t.p, axis=1) for t, ft in zip(new_terms, fit.terms)])
    assert unseen.any() and not unseen.all()
    if sample_new:
        assert ix.min() >= 0 and ix.max() >= q and coef[0].shape[1] > q          # unseen levels: extra columns behind the chain's b table
        assert np.all(ix[unseen] >= q) and np.all(ix[~unseen] < q)
    else:
        assert np.all(ix[unseen] == -1) and np.all(ix[~unseen] >= 0) and coef[0].shape == (5, q)          # padding is index -1
    for c in range(2):
        assert coef[c].shape[0] == 5 and np.array_equal(coef[c][:, :q], fit.stan[fit._rows("b.")][:, :, c].T)
        got = np.zeros((rows, 5))
        for e in range(ix.shape[1]):
            on = ix[:, e] >= 0
            got[on] += val[on, e][:, None] * coef[c][:, ix[on, e]].T
        np.testing.assert_allclose(got, want[:, :, c], rtol=1e-12, atol=1e-12)


class _NoSampler:
    def predict_summary(self, *a, **k):
        raise AssertionError("the ABI was called although the arguments had to be refused")


def test_python_refusals():
    fit, new_terms, _ = sc.fake_fit(0, samplers=[_NoSampler(), _NoSampler()])
    x = np.zeros((40, 3))
    with pytest.raises(ValueError, match="ppd"):
        fit.predict_summary(x_bart=x, type="ppd")
    with pytest.raises(ValueError, match="indiv.bart"):
        fit.predict_summary(x_bart=x, type="indiv.ranef")
    with pytest.raises(ValueError, match=r"shape \[G, 40\]"):
        fit.predict_summary(x_bart=x, row_weights=np.ones((2, 39)))
    with pytest.raises(ValueError, match=r"shape \[G, 40\]"):
        fit.predict_summary(x_bart=x, row_weights=np.ones(40))
    with pytest.raises(ValueError, match="9 weight vectors"):
        fit.predict_summary(x_bart=x, row_weights=np.ones((9, 40)))
    with pytest.raises(ValueError, match="x_bart"):
        fit.predict_summary(X=np.zeros((40, 2)))
    bare, _, _ = sc.fake_fit(0)
    with pytest.raises(ValueError, match="keepTrees"):
        bare.predict_summary(x_bart=x)


def test_entry_is_refused_on_the_emulated_layer(emul_lib):
    """The emulated device layer has no summary kernel: the C entry exists, answers the query for the number of kept draws, and refuses the call itself
    with a message; Python raises what abi.py raises elsewhere."""
    from stan4bart_amd.abi import StoredSampler
    assert hasattr(emul_lib, "emu_predict_summary")
    args, _ = friedman_case(n=100, T=5, warmup=3, iter=6, ranef=False)
    args.keep_trees = True
    s = make_sampler(emul_lib, "emu_", args)
    try:
        s.run(3, True)
        s.disengage_adaptation()
        s.run(3, False)
        x = np.asarray(args.x_bart)[:7]
        before = s.get_counters()
        with pytest.raises(RuntimeError, match="no summary kernel"):
            s.predict_summary(x)
        assert s.summary_info["launches"] == 0 and np.array_equal(s.get_counters(), before)
        with pytest.raises(ValueError, match="dense has 2 columns, dense_coef 3"):
            s.predict_summary(x, dense=np.zeros((7, 2)), dense_coef=np.zeros((3, 3)))
        with pytest.raises(ValueError, match="weights must be"):
            s.predict_summary(x, weights=np.ones(7))
        st = StoredSampler(emul_lib, "emu_", s.export_bart_state())
        try:
            with pytest.raises(RuntimeError, match="no summary kernel"):
                st.predict_summary(x)
        finally:
            st.free()
    finally:
        s.free()


def test_oracle_library_has_no_entry(oracle_lib):
    from stan4bart_amd.abi import Sampler
    s = Sampler.__new__(Sampler)
    s._lib, s._pfx = oracle_lib, "orc_"
    with pytest.raises(RuntimeError, match="no predict_summary"):
        Sampler.predict_summary(s, np.zeros((2, 3)))
