"""s4b_predict_contrast without a GPU: the model of tests/contrast_cases.py against a brute-force numpy loop over the emulated layer's predict_bart,
the differing-column rule (bins, not raw values) and the tree order on handwritten trees, the argument handling of Stan4bartFit.predict_contrast over
stand-in samplers, and the entry on the emulated device layer (no such kernels there: refused with its own message).  predict_quantiles' pooling moved
into helpers of SamplerCore that both entries call; on the emulated layer both entries are refused in front of them, so what this file can hold of
predict_quantiles is its unchanged refusal — its bits and the messages of its peer rules are held by tests/test_gpu_predict_quantiles.py, unchanged.
The kernels are tested in tests/test_gpu_predict_contrast.py."""
import numpy as np
import pytest

import contrast_cases as cc
import pd_cases as pc
import summary_cases as sc
from conftest import friedman_case

PROBS = (0.025, 0.5, 0.975, 0.0, 1.0)


@pytest.fixture(scope="module")
def emul_chain(emul_lib):
    args, _ = friedman_case(n=100, T=5, warmup=3, iter=6, ranef=False)
    args.keep_trees = True
    c = pc.Chain(emul_lib, "emu_", args, steps=(1, 2), rows=60)
    yield c
    c.close()


def _parts(chain, pool, x1, x0, cols, tables=None):
    parts = []
    for j, S in enumerate(pool):
        hit = chain.hit(S, cols) if len(cols) else np.zeros((S, chain.T), dtype=bool)
        F1, G1 = cc.leaf_sums(chain.trees[S], x1, hit)
        F0, G0 = cc.leaf_sums(chain.trees[S], x0, hit)
        parts.append(dict(bart1=chain.stored[S].predict_bart(x1), bart0=chain.stored[S].predict_bart(x0), F1=F1, F0=F0, G1=G1, G0=G0,
                          n_affected=hit.sum(axis=1), **(tables[j] if tables else {})))
    return parts


@pytest.mark.parametrize("link", [0, 1])
def test_model_against_a_brute_force_loop(emul_chain, link):
    ch, rows, pool = emul_chain, 60, (3, 1)
    x1 = np.asfortranarray(ch.x[:rows])
    x0 = x1.copy()
    x0[:, 0], x0[::3, 4] = x1[::-1, 0], 0.5
    w = sc.weight_vectors(rows, 3)
    ref, bd = cc.model(_parts(ch, pool, x1, x0, [0, 4]), {}, {}, ch.T, ch.range, ch.binary, link=link, weights=w, probs=PROBS)
    b1 = np.concatenate([ch.stored[S].predict_bart(x1) for S in pool], axis=1)
    b0 = np.concatenate([ch.stored[S].predict_bart(x0) for S in pool], axis=1)
    assert ref["d"].shape == (rows, 4) and np.any(b1 != b0)
    if link:
        b1, b0 = sc.phi_cdf(b1), sc.phi_cdf(b0)
    want = cc.brute_force(b1, b0, PROBS, w)
    np.testing.assert_allclose(ref["d"], b1 - b0, rtol=0, atol=1e-14)
    for key in ("mean", "m2", "average", "quantiles"):
        assert ref[key].shape == want[key].shape == bd[key].shape, key
        np.testing.assert_allclose(ref[key], want[key], rtol=1e-10, atol=1e-13, err_msg=key)
        assert np.all(bd[key] >= 0) and cc.bound_ratio(want[key], ref[key], bd[key] + 64 * cc.U * np.abs(ref[key]).max()) <= cc.BOUND_FACTOR, key


def test_model_with_linear_parts_that_differ_while_the_trees_do_not(emul_chain):
    ch, rows, S = emul_chain, 40, 3
    x = np.asfortranarray(ch.x[:rows])
    lp, lp0 = sc.linear_parts(rows, S, 3, 2), sc.linear_parts(rows, S, 3, 2, seed=9)
    arm1 = dict(offset=np.arange(rows) * 0.25, dense=lp["dense"], ell_index=lp["ell_index"], ell_value=lp["ell_value"])
    tables = [dict(dense_coef=lp["dense_coef"], ell_coef=lp["ell_coef"])]
    parts = _parts(ch, (S,), x, x, [], tables)
    same, bsame = cc.model(parts, arm1, {}, ch.T, ch.range, ch.binary)
    assert not same["d"].any() and not same["m2"].any() and not bsame["d"].any()          # identical arms: exactly 0, no allowance
    ref, bd = cc.model(parts, arm1, dict(dense=lp0["dense"]), ch.T, ch.range, ch.binary)
    want = (lp["dense"] - lp0["dense"]) @ lp["dense_coef"].T
    np.testing.assert_allclose(ref["d"], want, rtol=0, atol=1e-13)
    assert np.all(bd["d"] > 0) and np.all(bd["d"] < 1e-12)
    swapped, _ = cc.model(parts, dict(arm1, dense=lp0["dense"]), dict(dense=lp["dense"]), ch.T, ch.range, ch.binary)
    assert np.array_equal(swapped["d"], -ref["d"]) and np.array_equal(swapped["m2"], ref["m2"])
    ix0 = np.roll(lp["ell_index"], 1, axis=0)
    ref2, _ = cc.model(parts, arm1, dict(ell_index=ix0), ch.T, ch.range, ch.binary)
    full, differs = cc.resolve_arm0(arm1, dict(ell_index=ix0))
    assert differs == dict(offset=False, dense=False, ell=True) and full["ell_value"] is arm1["ell_value"] and ref2["d"].any()


def test_differing_columns_are_those_whose_bins_differ():
    cuts = [np.array([0.25, 0.5, 0.75]), np.array([1.0]), np.array([]), np.array([0.0, 10.0])]
    x1 = np.array([[0.1, 0.0, 3.0, -1.0], [0.5, 2.0, 4.0, 5.0], [0.9, 1.0, 5.0, 11.0]])
    assert np.array_equal(cc.bins(x1, cuts), [[0, 0, 0, 0], [1, 1, 0, 1], [3, 0, 0, 2]])          # a value ON a cut lies left of it
    x0 = x1.copy()
    x0[:, 0] = (0.2, 0.26, 0.76)          # other raw values inside the same bins
    x0[:, 2] = (-7.0, 0.0, 7.0)           # a column without cut points never differs
    x0[:, 3] = (-1e300, 10.0, np.inf)     # the ends
    assert cc.differing_columns(x1, x0, cuts) == []
    x0[1, 0] = np.nextafter(0.5, 1.0)     # one row crosses one cut
    assert cc.differing_columns(x1, x0, cuts) == [0]
    x0[2, 3] = 10.0
    x0[0, 1] = 1.5
    assert cc.differing_columns(x1, x0, cuts) == [0, 1, 3] and cc.differing_columns(x0, x1, cuts) == [0, 1, 3]


def test_tree_order_of_the_differing_columns_on_handwritten_trees():
    draws = [[[(0, 0.5), 1.0, 2.0], [3.0], [(2, 0.1), (1, 0.3), 1.0, 2.0, 3.0]],
             [[4.0], [(3, 0.5), 1.0, 2.0], [5.0]],
             [[(1, 0.5), 1.0, 2.0], [(0, 0.2), 1.0, (1, 0.7), 2.0, 3.0], [(1, 0.9), 1.0, 2.0]]]
    trees = pc.make_trees(draws)
    for cols, want_hit in (([1], [[0, 0, 1], [0, 0, 0], [1, 1, 1]]), ([0, 2], [[1, 0, 1], [0, 0, 0], [0, 1, 0]]), ([4], [[0] * 3] * 3)):
        hit = pc.affected(trees, cols, 3, 3)
        assert np.array_equal(hit, np.array(want_hit, dtype=bool)), cols
        order, n_base = pc.tree_order(hit)
        for k in range(3):          # unaffected trees first, then the affected ones, each group in ascending index
            assert sorted(order[k][:n_base[k]]) == list(order[k][:n_base[k]]) and sorted(order[k][n_base[k]:]) == list(order[k][n_base[k]:])
            assert not hit[k][order[k][:n_base[k]]].any() and hit[k][order[k][n_base[k]:]].all()
    # a draw with no affected tree, one whose trees are all affected: what the GPU cases must contain
    assert pc.affected(trees, [1], 3, 3).sum(axis=1).tolist() == [1, 0, 3]


def test_entry_is_refused_on_the_emulated_layer(emul_lib, emul_chain):
    assert hasattr(emul_lib, "emu_predict_contrast")
    x = emul_chain.x[:7]
    x0 = x.copy()
    x0[:, 1] = x[::-1, 1]
    for smp in (emul_chain.live, emul_chain.stored[3]):
        before = emul_chain.live.get_counters()
        with pytest.raises(RuntimeError, match="predict_contrast: this device layer has no contrast kernels"):
            smp.predict_contrast(x, x0, probs=[0.025, 0.975])
        with pytest.raises(RuntimeError, match="no contrast kernels"):
            smp.predict_contrast(x, x0, weights=np.ones((2, 7)), peers=[emul_chain.stored[1]], per_row=False)
        assert smp.contrast_info["launches"] == 0 and not any(smp.contrast_info.values()) and np.array_equal(emul_chain.live.get_counters(), before)
        with pytest.raises(RuntimeError, match="no quantile kernels"):          # the sibling's refusal is what it was
            smp.predict_quantiles(x, [0.5], peers=[emul_chain.stored[1]])
        with pytest.raises(ValueError, match="probs must be a vector"):
            smp.predict_contrast(x, x0, probs=[[0.5, 0.6]])
        with pytest.raises(ValueError, match=r"x_test0 must have shape \(7, 9\)"):
            smp.predict_contrast(x, x0[:5])
        with pytest.raises(ValueError, match="one table per peer"):
            smp.predict_contrast(x, x0, peers=[emul_chain.stored[1]], dense=np.ones((7, 2)), dense_coef=np.ones((3, 2)), peer_dense_coef=[])


def test_oracle_library_has_no_entry(oracle_lib):
    from stan4bart_amd.abi import Sampler
    s = Sampler.__new__(Sampler)
    s._lib, s._pfx = oracle_lib, "orc_"
    with pytest.raises(RuntimeError, match="no predict_contrast"):
        Sampler.predict_contrast(s, np.zeros((2, 3)))


class _Recorder:
    """A stand-in sampler: records the call and answers with zeros of the right shapes over 15 pooled draws."""

    def __init__(self, draws=15):
        self.calls, self.draws = [], draws

    def predict_contrast(self, x, x0, **kw):
        self.calls.append(dict(x=x, x0=x0, **kw))
        G, rows = kw["weights"].shape[0], len(x)
        avg = np.arange(self.draws * G, dtype=np.float64).reshape(self.draws, G)
        return dict(mean=np.zeros(rows), m2=np.full(rows, 14.0), average=avg, quantiles=np.zeros((len(kw["probs"]), rows)), draws=self.draws, info={})


class _NoSampler:
    def predict_contrast(self, *a, **k):
        raise AssertionError("the ABI was called although the arguments had to be refused")


def test_python_refusals():
    fit, new_terms, _ = sc.fake_fit(0, samplers=[_NoSampler(), _NoSampler()])
    x = np.zeros((40, 3))
    with pytest.raises(ValueError, match="predict_contrast does not form 'ppd'"):
        fit.predict_contrast(x, type="ppd")
    for t in ("indiv.fixef", "indiv.ranef"):
        with pytest.raises(ValueError, match="indiv.fixef and indiv.ranef need no trees: use predict"):
            fit.predict_contrast(x, type=t)
    with pytest.raises(ValueError, match="predict_contrast needs x_bart"):
        fit.predict_contrast()
    for bad in ((-0.1, 0.5), (0.5, 1.5), (np.nan,), ((0.1, 0.2),), np.linspace(0, 1, 17)):
        with pytest.raises(ValueError, match=r"'probs' must be a vector of at most 16 values in \[0, 1\]"):
            fit.predict_contrast(x, probs=bad)
    for arm0 in (dict(x_bart0=x), dict(X0=np.zeros((40, 2))), dict(groups0=new_terms), dict(offset0=np.zeros(40))):
        with pytest.raises(ValueError, match="'treatment' builds both arms from one row set: no explicit arm-0 argument"):
            fit.predict_contrast(x, treatment=("x_bart", 1), **arm0)
    for bad in ("x_bart", ("Z", 0), ("x_bart", 0, 1)):
        with pytest.raises(ValueError, match="'treatment' must be"):
            fit.predict_contrast(x, treatment=bad)
    with pytest.raises(ValueError, match="names column 3 of x_bart, which is not there"):
        fit.predict_contrast(x, treatment=("x_bart", 3))
    with pytest.raises(ValueError, match="names column 0 of X, which is not there"):
        fit.predict_contrast(x, treatment=("X", 0))
    with pytest.raises(ValueError, match="X0 given without X"):
        fit.predict_contrast(x, X0=np.zeros((40, 2)))
    with pytest.raises(ValueError, match="groups0 given without groups"):
        fit.predict_contrast(x, groups0=new_terms)
    with pytest.raises(ValueError, match="offset0 given without offset"):
        fit.predict_contrast(x, offset0=np.zeros(40))
    with pytest.raises(ValueError, match=r"row_weights must have shape \[G, 40\]"):
        fit.predict_contrast(x, row_weights=np.ones(40))
    with pytest.raises(ValueError, match="row_weights holds 9 weight vectors"):
        fit.predict_contrast(x, row_weights=np.ones((9, 40)))
    bare, _, _ = sc.fake_fit(0)
    with pytest.raises(ValueError, match="predict_contrast requires 'bart_args' to contain 'keepTrees'"):
        bare.predict_contrast(x)


def test_one_pooled_call_with_both_arms_through_one_stacked_ell_table():
    from stan4bart_amd import GroupTerm
    a, b, c = _Recorder(), _NoSampler(), _NoSampler()          # the first sampler takes the call, the others travel as its peers
    fit, new_terms, q = sc.fake_fit(0, n_chain=3, samplers=[a, b, c])
    g = np.random.default_rng(4)
    x, X, off = g.normal(size=(40, 3)), g.normal(size=(40, 2)), g.normal(size=40)
    x0, X0, off0 = g.normal(size=(40, 3)), g.normal(size=(40, 2)), g.normal(size=40)
    # arm 0: other slopes, and other levels in the last term
    terms0 = [GroupTerm(t.levels if j < 2 else np.roll(t.levels, 1), None if t.slopes is None else t.slopes + 1.0, t.name) for j, t in enumerate(new_terms)]
    out = fit.predict_contrast(x, x0, X=X, X0=X0, groups=new_terms, groups0=terms0, offset=off, offset0=off0, seed=5)
    assert out["draws"] == 15 and out["average"].shape == (1, 15) and out["quantiles"].shape == (3, 40) and np.array_equal(out["probs"], (0.025, 0.5, 0.975))
    np.testing.assert_array_equal(out["sd"], 1.0)
    call = a.calls[0]
    assert len(a.calls) == 1 and call["peers"] == [b, c] and np.array_equal(call["x"], x) and np.array_equal(call["x0"], x0)
    assert np.array_equal(call["weights"], np.full((1, 40), 1 / 40)) and call["link"] == 0
    assert np.array_equal(call["dense"], X - fit.X_means) and np.array_equal(call["dense0"], X0 - fit.X_means)
    assert np.array_equal(call["offset"], off) and np.array_equal(call["offset0"], off0)
    # ONE _ell_random call on the stacked rows: one table, one draw of every unseen level for both arms
    stacked = [GroupTerm(np.concatenate([t.levels, t0.levels]), None if t.slopes is None else np.vstack([t.slopes, t0.slopes]), t.name)
               for t, t0 in zip(new_terms, terms0)]
    ix, val, coef = fit._ell_random(stacked, True, np.random.default_rng(5))
    assert ix.max() >= q, "no unseen level reached the table"
    assert np.array_equal(call["ell_index"], ix[:40]) and np.array_equal(call["ell_index0"], ix[40:])
    assert np.array_equal(call["ell_value"], val[:40]) and np.array_equal(call["ell_value0"], val[40:])
    assert np.array_equal(call["ell_coef"], coef[0]) and all(np.array_equal(p, w) for p, w in zip(call["peer_ell_coef"], coef[1:]))
    beta = fit.stan[fit._rows("beta.")]
    assert np.array_equal(call["dense_coef"], beta[:, :, 0].T) and np.array_equal(call["peer_dense_coef"][1], beta[:, :, 2].T)
    # chains apart: [G, iter, chain], chain after chain in the pooled order
    a.calls.clear()
    w = sc.weight_vectors(40, 2)
    apart = fit.predict_contrast(x, x0, row_weights=w, combine_chains=False, probs=())
    assert apart["average"].shape == (2, 5, 3) and apart["quantiles"].shape == (0, 40)
    pooled = np.arange(30.0).reshape(15, 2).T
    assert all(np.array_equal(apart["average"][:, :, ch], pooled[:, 5 * ch:5 * ch + 5]) for ch in range(3))
    call = a.calls[0]
    assert call.get("dense") is None and call.get("ell_index") is None and call["offset"] is None and call["peer_dense_coef"] is None


def test_treatment_builds_both_arms_from_one_row_set():
    a = _Recorder(5)
    fit, new_terms, _ = sc.fake_fit(0, n_chain=1, family="binomial", samplers=[a])
    g = np.random.default_rng(6)
    x, X = g.normal(size=(40, 3)), g.normal(size=(40, 2))
    fit.predict_contrast(x, X=X, groups=new_terms, treatment=("x_bart", 2), seed=3)
    call = a.calls[0]
    assert np.array_equal(call["x"][:, 2], np.ones(40)) and not call["x0"][:, 2].any() and np.array_equal(call["x"][:, :2], x[:, :2]) and np.array_equal(call["x0"][:, :2], x[:, :2])
    assert call["link"] == 1 and call["dense0"] is None and call.get("ell_index0") is None and call["ell_index"] is not None
    fit.predict_contrast(x, X=X, treatment=("X", 1), levels=(2.0, -1.0), type="ev")
    call = a.calls[1]
    assert call["x0"] is None and np.array_equal(call["dense"][:, 1], 2.0 - np.full(40, fit.X_means[1])) and np.array_equal(call["dense0"][:, 1], -1.0 - np.full(40, fit.X_means[1]))
    assert np.array_equal(call["dense"][:, 0], call["dense0"][:, 0])
    # the same bits as the explicit arms
    x1, x0 = x.copy(), x.copy()
    x1[:, 2], x0[:, 2] = 1.0, 0.0
    fit.predict_contrast(x1, x0, X=X, groups=new_terms, seed=3)
    assert all(np.array_equal(a.calls[2][k], a.calls[0][k]) for k in ("x", "x0", "dense", "ell_index", "ell_value", "ell_coef", "weights"))
