"""s4b_partial_dependence without a GPU: the model of tests/pd_cases.py against a plain numpy loop over the emulated layer's predict_bart, the
tree-order restatement on handwritten trees, the grid handling of Stan4bartFit.partial_dependence (default grid, product grid, chunks of 64 joined in
order, refusals) over stand-in samplers, and the entry on the emulated device layer (no such kernel there: refused with its message).  The kernels
are tested in tests/test_gpu_partial_dependence.py."""
import numpy as np
import pytest

import pd_cases as pc
import summary_cases as sc
from conftest import friedman_case


def test_tree_order_on_handwritten_trees():
    leaf = [0.5]
    root_on_2 = [(2, 0.1), -1.0, 1.0]
    below_root = [(0, 0.3), 0.25, (2, 0.7), -0.5, 0.5]          # a rule on predictor 2 only below the root
    on_0 = [(0, 0.3), 0.25, 0.75]
    trees = pc.make_trees([[leaf, on_0, leaf, on_0, leaf],                          # draw 0: no tree holds a rule on 2
                           [root_on_2, below_root, root_on_2, below_root, root_on_2],  # draw 1: all do
                           [on_0, below_root, leaf, root_on_2, on_0]])              # draw 2: trees 1 and 3
    hit = pc.affected(trees, 2, 3, 5)
    assert hit.tolist() == [[False] * 5, [True] * 5, [False, True, False, True, False]]
    order, num_base = pc.tree_order(hit)
    assert order.tolist() == [[0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [0, 2, 4, 1, 3]] and num_base.tolist() == [5, 0, 3]
    # two varied predictors: a tree with a rule on either is affected; a predictor no tree uses changes nothing
    hit02 = pc.affected(trees, [0, 2], 3, 5)
    assert hit02.tolist() == [[False, True, False, True, False], [True] * 5, [True, True, False, True, True]]
    assert pc.tree_order(hit02)[0].tolist() == [[0, 2, 4, 1, 3], [0, 1, 2, 3, 4], [2, 0, 1, 3, 4]]
    assert np.array_equal(pc.affected(trees, [2, 7], 3, 5), hit) and not pc.affected(trees, 7, 3, 5).any()
    for h in (hit, hit02):          # a permutation of the trees in every draw, each group ascending
        o, nb = pc.tree_order(h)
        for k in range(3):
            assert sorted(o[k]) == list(range(5)) and list(o[k, :nb[k]]) == sorted(o[k, :nb[k]]) and list(o[k, nb[k]:]) == sorted(o[k, nb[k]:])
            assert not h[k, o[k, :nb[k]]].any() and h[k, o[k, nb[k]:]].all()


@pytest.fixture(scope="module")
def emul_chain(emul_lib):
    args, _ = friedman_case(n=100, T=5, warmup=3, iter=6, ranef=False)
    args.keep_trees = True
    c = pc.Chain(emul_lib, "emu_", args, steps=(1, 2), rows=60)
    yield c
    c.close()


def test_model_matches_a_plain_numpy_loop(emul_chain):
    c = emul_chain
    S, rows = 3, 60
    per_var = [int(pc.affected(c.trees[S], v, S, c.T).sum()) for v in range(c.P)]
    v0, v1 = int(np.argmax(per_var)), int(np.argsort(per_var)[-2])
    assert per_var[v0] > 0
    lo, hi = c.args.x_bart[:, v0].min(), c.args.x_bart[:, v0].max()
    grid = np.r_[-np.inf, np.linspace(lo, hi, 5), np.inf]
    w = sc.weight_vectors(rows, 3)[2]
    for weights in (None, w):
        ref, bound = c.reference(S, rows, v0, grid, weights=weights)
        brute = pc.brute_force(c.stored[S].predict_bart, c.x[:rows], v0, grid, weights)
        assert ref.shape == (S, len(grid)) and np.all(bound > 0)
        np.testing.assert_allclose(ref, brute, rtol=1e-12, atol=1e-13)
        assert len({tuple(col) for col in ref.T}) > 1, "the grid moves nothing: the case tests no partial dependence"
    pair = np.column_stack([np.repeat(grid[1:4], 2), np.tile([lo, hi], 3)])
    ref2, _ = c.reference(S, rows, [v0, v1], pair)
    np.testing.assert_allclose(ref2, pc.brute_force(c.stored[S].predict_bart, c.x[:rows], [v0, v1], pair), rtol=1e-12, atol=1e-13)
    # the linear parts stay at the rows' own values: with link 0 they shift every grid point of a draw by the same weighted sum
    parts = sc.linear_parts(rows, S, 2, 2, seed=1)
    off = np.random.default_rng(0).normal(size=rows)
    ref3, bound3 = c.reference(S, rows, v0, grid, offset=off, **parts)
    lin, _ = sc.model(np.zeros((rows, S)), off, weights=np.full((1, rows), 1.0 / rows), **parts)
    base, _ = c.reference(S, rows, v0, grid)
    np.testing.assert_allclose(ref3, base + lin["average"], rtol=1e-12, atol=1e-13)
    assert np.all(bound3 > 0)
    ref4, bound4 = c.reference(S, rows, v0, grid, offset=off, link=1, **parts)          # link 1: values in (0, 1), the order term carried through phi
    assert np.all((ref4 > 0) & (ref4 < 1)) and np.all(bound4 >= sc.ERFC_C * sc.U * 0.999)


def test_entry_is_refused_on_the_emulated_layer(emul_lib, emul_chain):
    assert hasattr(emul_lib, "emu_partial_dependence")
    x = emul_chain.x[:7]
    for smp in (emul_chain.live, emul_chain.stored[3]):
        before = emul_chain.live.get_counters()
        with pytest.raises(RuntimeError, match="no partial-dependence kernel"):
            smp.partial_dependence(x, 0, [0.25, 0.5])
        assert smp.pd_info["launches"] == 0 and smp.pd_info["route"] == 0 and np.array_equal(emul_chain.live.get_counters(), before)
        with pytest.raises(ValueError, match="vars must be one predictor index or two"):
            smp.partial_dependence(x, [0, 1, 2], [0.5])
        with pytest.raises(ValueError, match=r"grid must be \[G\] or \[G x 2\]"):
            smp.partial_dependence(x, [0, 1], [0.25, 0.5, 0.75])


def test_oracle_library_has_no_entry(oracle_lib):
    from stan4bart_amd.abi import Sampler
    s = Sampler.__new__(Sampler)
    s._lib, s._pfx = oracle_lib, "orc_"
    with pytest.raises(RuntimeError, match="no partial_dependence"):
        Sampler.partial_dependence(s, np.zeros((2, 3)), 0, [0.5])


class _Recorder:
    """A stand-in sampler: records every call and answers pd[k, g] = 1000 k + (first grid value of g) + 0.5 (second)."""

    def __init__(self, draws=4):
        self.draws, self.calls = draws, []

    def partial_dependence(self, x, vars, grid, **kw):
        grid = np.asarray(grid)
        self.calls.append(dict(vars=list(vars), grid=grid.copy(), **kw))
        assert len(grid) <= 64
        g = grid[:, 0] + (0.5 * grid[:, 1] if grid.shape[1] > 1 else 0.0)
        return dict(pd=1000.0 * np.arange(self.draws)[:, None] + g[None, :], draws=self.draws, info={})


class _NoSampler:
    def partial_dependence(self, *a, **k):
        raise AssertionError("the ABI was called although the arguments had to be refused")


def test_default_grid_chunks_and_joining():
    from stan4bart_amd.generics import PD_LEVQUANTS, Stan4bartFit
    assert PD_LEVQUANTS == (0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95)
    g = np.random.default_rng(4)
    x = g.normal(size=(40, 3))
    a, b = _Recorder(5), _Recorder(5)
    fit, _, _ = sc.fake_fit(0, samplers=[a, b])
    out = fit.partial_dependence(1, x, type="indiv.bart")
    want = np.quantile(x[:, 1], PD_LEVQUANTS)
    assert np.array_equal(out["grid"], want) and np.array_equal(Stan4bartFit.pd_default_grid(x[:, 1]), want)
    assert len(a.calls) == len(b.calls) == 1 and a.calls[0]["vars"] == [1] and np.array_equal(a.calls[0]["grid"][:, 0], want)
    assert a.calls[0]["weights"] is None and a.calls[0]["link"] == 0 and a.calls[0]["dense"] is None and a.calls[0]["ell_index"] is None
    assert out["pd"].shape == (11, 10) and np.array_equal(out["pd"][:, 3], 3000.0 + want) and np.array_equal(out["pd"][:, 5], want)
    np.testing.assert_allclose(out["mean"], out["pd"].mean(axis=1))
    lo, hi = np.quantile(out["pd"], (0.025, 0.975), axis=1)
    assert np.array_equal(out["lower"], lo) and np.array_equal(out["upper"], hi)
    split = fit.partial_dependence(1, x, type="indiv.bart", combine_chains=False)
    assert split["pd"].shape == (11, 5, 2) and np.array_equal(split["pd"][:, :, 1], out["pd"][:, 5:])
    # 150 grid points: calls of 64, 64 and 22, joined in the grid's order
    a.calls.clear()
    long = np.sort(g.normal(size=150))[::-1]
    out = fit.partial_dependence(2, x, grid=long, type="indiv.bart", probs=(0.25, 0.75))
    assert [len(c["grid"]) for c in a.calls] == [64, 64, 22] and np.array_equal(np.concatenate([c["grid"][:, 0] for c in a.calls]), long)
    assert out["pd"].shape == (150, 10) and np.array_equal(out["pd"][:, 1], 1000.0 + long)
    assert np.array_equal(out["lower"], np.quantile(out["pd"], 0.25, axis=1))
    # a pair of predictors: the default grid is the product of the two columns' quantiles, first predictor slowest, 121 points in two calls
    a.calls.clear()
    out = fit.partial_dependence((2, 0), x, type="indiv.bart")
    q2, q0 = np.quantile(x[:, 2], PD_LEVQUANTS), np.quantile(x[:, 0], PD_LEVQUANTS)
    assert out["grid"].shape == (121, 2) and np.array_equal(out["grid"][:, 0], np.repeat(q2, 11)) and np.array_equal(out["grid"][:, 1], np.tile(q0, 11))
    assert [len(c["grid"]) for c in a.calls] == [64, 57] and a.calls[0]["vars"] == [2, 0]
    assert np.array_equal(out["pd"][:, 0], out["grid"][:, 0] + 0.5 * out["grid"][:, 1])
    # the linear parts are predict_summary's: the same tables reach the sampler, weights as one vector
    _, new_terms, _ = sc.fake_fit(0)
    a.calls.clear()
    w = g.uniform(size=40)
    X = g.normal(size=(40, 2))
    fit.partial_dependence(0, x, grid=[0.0, 1.0], X=X, groups=new_terms, offset=np.ones(40), row_weights=w, seed=5)
    ix, val, coef = fit._ell_random(new_terms, True, np.random.default_rng(5))
    call = a.calls[0]
    assert np.array_equal(call["ell_index"], ix) and np.array_equal(call["ell_value"], val) and np.array_equal(call["ell_coef"], coef[0])
    assert np.array_equal(b.calls[-1]["ell_coef"], coef[1]) and np.array_equal(call["dense"], X - fit.X_means) and np.array_equal(call["weights"], w)
    assert np.array_equal(call["offset"], np.ones(40)) and call["link"] == 0


def test_python_refusals():
    fit, _, _ = sc.fake_fit(0, samplers=[_NoSampler(), _NoSampler()])
    x = np.zeros((40, 3))
    with pytest.raises(ValueError, match="ppd"):
        fit.partial_dependence(0, x, type="ppd")
    with pytest.raises(ValueError, match="indiv.bart"):
        fit.partial_dependence(0, x, type="indiv.fixef")
    for bad in (3, -1, (0, 0), (0, 1, 2)):
        with pytest.raises(ValueError, match="'var' must be one column index"):
            fit.partial_dependence(bad, x)
    with pytest.raises(ValueError, match="NaN"):
        fit.partial_dependence(0, x, grid=[0.0, np.nan])
    with pytest.raises(ValueError, match="at least one point"):
        fit.partial_dependence(0, x, grid=[])
    with pytest.raises(ValueError, match="at least one point of 2"):
        fit.partial_dependence((0, 1), x, grid=[0.0, 1.0, 2.0])
    with pytest.raises(ValueError, match=r"row_weights must have shape \[40\]"):
        fit.partial_dependence(0, x, row_weights=np.ones((2, 40)))
    with pytest.raises(ValueError, match="x_bart"):
        fit.partial_dependence(0)
    bare, _, _ = sc.fake_fit(0)
    with pytest.raises(ValueError, match="keepTrees"):
        bare.partial_dependence(0, x)
