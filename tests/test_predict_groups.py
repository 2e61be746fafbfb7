"""s4b_predict_groups without a GPU (tests/group_cases.py: the model, the bound, the labels): the model against a brute-force numpy loop over the
emulated layer's predict_bart, the binding's stable sort and its inverse mapping, the refusal on the emulated device layer, the absence from the
oracle library, the refusals of the Python method and the arithmetic of the level ranges.

test_model_against_a_brute_force_loop and test_labels_put_the_cases_of_the_reduction_next_to_one_another guard the MODEL and the labels of
tests/group_cases.py, which the device tests are measured against, not the product: they use group_cases and the emulated predict_bart alone."""
import numpy as np
import pytest

import group_cases as gc
import pd_cases as pc
import summary_cases as sc
from conftest import friedman_case

PROBS = (0.025, 0.5, 0.975, 0.0, 1.0)


@pytest.fixture(scope="module")
def emul_chain(emul_lib):
    args, _ = friedman_case(n=100, T=5, warmup=3, iter=6, ranef=False)
    args.keep_trees = True
    c = pc.Chain(emul_lib, "emu_", args, steps=(1, 2), rows=200)
    yield c
    c.close()


@pytest.mark.parametrize("statistic", [0, 1])
def test_model_against_a_brute_force_loop(emul_chain, statistic):
    ch, rows = emul_chain, 200
    x = np.concatenate([ch.stored[3].predict_bart(ch.x), ch.stored[1].predict_bart(ch.x)], axis=1)          # [rows x 4]: the pool (3, 1)
    level, L = gc.slab_labels(rows)
    w = np.random.default_rng(1).uniform(0.0, 2.0, rows)
    w[64:128] = 0.0          # a level whose weights are all 0
    ref, bd = gc.model(x, np.zeros_like(x), level, L, w, statistic, PROBS)
    want = gc.brute_force(x, level, L, w, statistic)
    assert np.array_equal(np.isnan(ref["draws"]), np.isnan(want)) and np.isnan(ref["draws"][0, 0]) and np.isnan(ref["draws"][L - 1, 0])
    assert np.isnan(ref["draws"][3, 0]) == (statistic == 1) and (statistic == 1 or np.all(ref["draws"][3] == 0.0))
    ok = ~np.isnan(want[:, 0])
    np.testing.assert_allclose(ref["draws"][ok], want[ok], rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(ref["mean"][ok], want[ok].mean(axis=1), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(ref["m2"][ok], ((want[ok] - want[ok].mean(axis=1, keepdims=True)) ** 2).sum(axis=1), rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(ref["quantiles"][:, ok], np.quantile(want[ok], PROBS, axis=1), rtol=1e-12, atol=1e-13)
    assert np.array_equal(ref["count"], np.bincount(level, minlength=L)) and ref["weight"][3] == 0.0 and ref["weight"][1] == w[0]
    # with exact inputs the bound is the reduction's own: (min(n, 64) + ceil(n / 64) + 1) u sum |w x| (+ u |A| for the division)
    n = 150
    i0 = int(np.flatnonzero(level == 5)[0])
    assert np.sum(level == 5) == min(n, rows - i0)
    n = int(np.sum(level == 5))
    sums = (w[i0:i0 + n, None] * np.abs(x[i0:i0 + n])).sum(axis=0)
    if statistic == 0:
        np.testing.assert_allclose(bd["draws"][5], (min(n, 64) + -(-n // 64) + 1) * gc.U * sums, rtol=1e-12)
    else:
        np.testing.assert_allclose(bd["draws"][5], (min(n, 64) + -(-n // 64) + 1) * gc.U * sums / ref["weight"][5] + gc.U * np.abs(ref["draws"][5]), rtol=1e-12)
    # thresholds: midway between two adjacent values nothing is ambiguous, on a value everything with that value is
    t = gc.midway(ref["draws"])
    r2, _ = gc.model(x, np.full_like(x, 1e-18), level, L, w, statistic, threshold=t)
    assert r2["ambiguous"] == 0 and np.array_equal(r2["p_above"][ok], (want[ok] > t).mean(axis=1)) and np.all(np.isnan(r2["p_above"][~ok]))
    r3, _ = gc.model(x, np.full_like(x, 1e-18), level, L, w, statistic, threshold=float(ref["draws"][1, 0]))
    assert r3["ambiguous"] >= 1
    assert gc.model(x, np.zeros_like(x), level, L, w, statistic, threshold=np.inf)[0]["ambiguous"] == 0


def test_labels_put_the_cases_of_the_reduction_next_to_one_another():
    for rows, edges in ((63, 0), (64, 0), (65, 0), (129, 0), (1100, 2 + sum(1 for i in range(978, 1100, 2) if i // 64 != (i + 1) // 64))):
        level, L = gc.slab_labels(rows)
        st = gc.level_starts(level, L)
        assert len(level) == rows and st[0] == st[1] == 0 and st[L] == st[L - 1] == rows, "an empty level at either end"
        assert st[2] - st[1] == 1, "a level of one row"
        assert gc.edge_levels(level, L) == edges, (rows, gc.edge_levels(level, L))
        if rows >= 65:
            assert st[3] == 64 and level[63] == 2 and level[64] == 3, "a level that ends on row 63 and the next that starts on row 64"
            assert st[5] == st[4], "an empty level in the middle"
        if rows == 1100:
            assert (st[3], st[4]) == (64, 128) and (st[5], st[6]) == (128, 278) and st[7] == 978, "one slab exactly; three slabs; over many chunks of 64 rows"
    assert gc.host_weight([0.1] * 10) == sum([0.1] * 10) != 1.0          # the host's W_l: in row order, in double


def test_stable_sort_and_inverse_mapping_of_the_binding():
    from stan4bart_amd.abi import Sampler
    g = np.random.default_rng(2)
    lab = g.integers(0, 7, 500)
    order, sorted_lab = Sampler.group_order(lab)
    assert np.array_equal(sorted_lab, lab[order]) and np.all(np.diff(sorted_lab) >= 0)
    for l in range(7):          # stable: the rows of a level keep their given order
        assert np.array_equal(order[sorted_lab == l], np.flatnonzero(lab == l))
    assert np.array_equal(np.sort(order), np.arange(500))
    with pytest.raises(ValueError, match="vector of integers"):
        Sampler.group_order(np.array([0.5, 1.0]))


def test_entry_is_refused_on_the_emulated_layer(emul_lib, emul_chain):
    assert hasattr(emul_lib, "emu_predict_groups")
    x = emul_chain.x[:7]
    level = np.array([2, 0, 1, 1, 0, 2, 2])
    for smp in (emul_chain.live, emul_chain.stored[3]):
        assert smp.groups_draws() == 3
        before = emul_chain.live.get_counters()
        with pytest.raises(RuntimeError, match="predict_groups: this device layer has no level kernels"):
            smp.predict_groups(x, level, 3, probs=[0.025, 0.975])
        with pytest.raises(RuntimeError, match="no level kernels"):
            smp.predict_groups(x, level, 3, x_test0=x[::-1], n_arms=2, weights=np.ones(7), peers=[emul_chain.stored[1]], threshold=0.0)
        assert not any(smp.groups_info.values()) and np.array_equal(emul_chain.live.get_counters(), before)
        with pytest.raises(RuntimeError, match="no contrast kernels"):          # the sibling's refusal is what it was
            smp.predict_contrast(x, x[::-1], probs=[0.5])
        with pytest.raises(ValueError, match="one integer per row"):
            smp.predict_groups(x, level[:5], 3)
        with pytest.raises(ValueError, match="one integer per row"):
            smp.predict_groups(x, level.astype(np.float64), 3)
        with pytest.raises(ValueError, match=r"weights must be \[7\]"):
            smp.predict_groups(x, level, 3, weights=np.ones((2, 7)))
        with pytest.raises(ValueError, match="unknown outputs"):
            smp.predict_groups(x, level, 3, outputs=("median",))


def test_oracle_library_has_no_entry(oracle_lib):
    from stan4bart_amd.abi import Sampler
    assert not hasattr(oracle_lib, "orc_predict_groups")
    s = Sampler.__new__(Sampler)
    s._lib, s._pfx = oracle_lib, "orc_"
    with pytest.raises(RuntimeError, match="no predict_groups"):
        Sampler.predict_groups(s, np.zeros((2, 3)), np.zeros(2, dtype=np.int64), 1)


class _Recorder:
    """A stand-in sampler of 15 draws: records the calls and answers with the level numbers over the pooled draws."""

    def __init__(self, draws=15):
        self.calls, self.draws = [], draws

    def groups_draws(self):
        return self.draws

    def predict_groups(self, **kw):
        self.calls.append(kw)
        L, Q, S = kw["n_levels"], len(kw["probs"]), self.draws * (1 + len(kw["peers"]))          # (the peers hold as many draws)
        base = float(len(self.calls)) * 100.0 + np.arange(L)
        return dict(mean=base.copy(), m2=np.full(L, 14.0), weight=np.bincount(kw["level"], weights=kw.get("weights"), minlength=L).astype(np.float64),
                    count=np.bincount(kw["level"], minlength=L), quantiles=np.tile(base, (Q, 1)), p_above=None if kw["threshold"] is None else base / 1e4,
                    draws=np.tile(base[:, None], (1, S)) if "draws" in kw["outputs"] else None, draws_pooled=S, info={})


class _NoSampler:
    def groups_draws(self):
        return 15

    def predict_groups(self, *a, **k):
        raise AssertionError("the ABI was called although the arguments had to be refused")


def test_python_refusals():
    fit, new_terms, _ = sc.fake_fit(0, samplers=[_NoSampler(), _NoSampler()])
    x, by = np.zeros((40, 3)), np.arange(40) % 3
    with pytest.raises(ValueError, match="predict_groups does not form 'ppd'"):
        fit.predict_groups(by, x, type="ppd")
    with pytest.raises(ValueError, match="indiv.fixef and indiv.ranef need no trees: use predict"):
        fit.predict_groups(by, x, type="indiv.ranef")
    with pytest.raises(ValueError, match="predict_groups needs x_bart"):
        fit.predict_groups(by)
    with pytest.raises(ValueError, match="'statistic' must be one of sum, mean"):
        fit.predict_groups(by, x, statistic="median")
    with pytest.raises(ValueError, match="at most 16 values in"):
        fit.predict_groups(by, x, probs=[1.5])
    with pytest.raises(ValueError, match="'threshold' is a NaN"):
        fit.predict_groups(by, x, threshold=np.nan)
    with pytest.raises(ValueError, match="'by' names the grouping term 'g.9', which is not in 'groups'"):
        fit.predict_groups("g.9", x, groups=new_terms)
    with pytest.raises(ValueError, match=r"'by' must hold one label per row \(40\)"):
        fit.predict_groups(by[:7], x)
    for bad in (np.full(40, -1.0), np.full(40, np.nan), np.full(40, np.inf), np.ones(39)):
        with pytest.raises(ValueError, match="row_weights must be .40. finite non-negative values"):
            fit.predict_groups(by, x, row_weights=bad)
    with pytest.raises(ValueError, match="'treatment' builds both arms from one row set"):
        fit.predict_groups(by, x, x_bart0=x, treatment=("x_bart", 0))
    with pytest.raises(ValueError, match="X0 given without X"):
        fit.predict_groups(by, x, X0=np.zeros((40, 2)))
    with pytest.raises(ValueError, match=r"level_bytes 100 does not hold one level of 30 pooled draws \(240 bytes\)"):
        fit.predict_groups(by, x, level_bytes=100)
    with pytest.raises(ValueError, match="level_bytes 300 holds one level of 30 pooled draws: a split needs room for two"):
        fit.predict_groups(by, x, level_bytes=300)
    none = sc.fake_fit(0)[0]
    with pytest.raises(ValueError, match="predict_groups requires 'bart_args' to contain 'keepTrees' as True"):
        none.predict_groups(by, x)


def test_level_range_split_arithmetic():
    from stan4bart_amd.abi import GROUPS_LEVEL_BYTES_MAX
    from stan4bart_amd.generics import Stan4bartFit
    assert GROUPS_LEVEL_BYTES_MAX == gc.LEVEL_BYTES_MAX == 1 << 30
    assert Stan4bartFit.groups_split(500, 400, 1 << 30) == [(0, 500)]
    assert Stan4bartFit.groups_split(3, 16, 8 * 16 * 3) == [(0, 3)]          # what fits goes in one call
    # a split: one level of the limit stays free for the rows in front of a range
    assert Stan4bartFit.groups_split(7, 16, 8 * 16 * 3) == [(0, 2), (2, 4), (4, 6), (6, 7)]
    assert Stan4bartFit.groups_split(6, 16, 8 * 16 * 3 + 127) == [(0, 2), (2, 4), (4, 6)]
    per = (1 << 30) // (8 * 16384) - 1
    assert Stan4bartFit.groups_split(20000, 16384, 1 << 30) == [(l, min(20000, l + per)) for l in range(0, 20000, per)] and per == 8191
    with pytest.raises(ValueError, match="does not hold one level"):
        Stan4bartFit.groups_split(5, 16, 127)
    with pytest.raises(ValueError, match="a split needs room for two"):
        Stan4bartFit.groups_split(5, 16, 255)


def test_ranges_are_slices_of_the_rows_sorted_by_level():
    a = _Recorder()
    fit, new_terms, _ = sc.fake_fit(0, n_chain=3, samplers=[a, _NoSampler(), _NoSampler()])
    g = np.random.default_rng(4)
    rows = 40
    x, X, off = g.normal(size=(rows, 3)), g.normal(size=(rows, 2)), g.normal(size=rows)
    names = np.array(["d", "b", "a", "e", "c"])
    by = names[g.integers(0, 5, rows)]
    w = g.uniform(0.5, 1.5, rows)
    got = fit.predict_groups(by, x, X=X, groups=new_terms, offset=off, row_weights=w, threshold=0.25, return_draws=True, seed=3, level_bytes=8 * 45 * 3)
    assert np.array_equal(got["levels"], ["a", "b", "c", "d", "e"]) and got["draws"] == 45 and len(a.calls) == 3
    code = np.searchsorted(got["levels"], by)
    order = np.argsort(code, kind="stable")
    start = np.searchsorted(code[order], np.arange(6))
    for j, call in enumerate(a.calls):
        l0, l1 = 2 * j, min(5, 2 * j + 2)
        i0, i1 = start[l0], start[l1]          # (40 rows: every range starts inside the first slab and takes the rows in front of it along as level 0)
        lead = 1 if i0 else 0
        assert call["n_levels"] == l1 - l0 + lead and call["presorted"] and call["n_arms"] == 1 and call["statistic"] == "mean" and call["threshold"] == 0.25
        assert np.array_equal(call["level"], np.r_[np.zeros(i0, dtype=np.int64), code[order[i0:i1]] - l0 + lead]) and np.all(np.diff(call["level"]) >= 0)
        rows_of = order[:i1]
        assert np.array_equal(call["x_test"], x[rows_of]) and np.array_equal(call["offset"], off[rows_of]) and np.array_equal(call["weights"], w[rows_of])
        assert np.array_equal(call["dense"], (X - fit.X_means)[rows_of]) and call["ell_index"].shape[0] == i1 and call["x_test0"] is None
        assert len(call["peers"]) == 2 and len(call["peer_dense_coef"]) == 2 and call["link"] == 0
    assert np.array_equal(got["mean"], [100.0, 101.0, 201.0, 202.0, 301.0]) and got["average"].shape == (5, 45)          # (level 0 of the later calls dropped)
    assert np.array_equal(got["count"], np.bincount(code)) and np.allclose(got["weight"], np.bincount(code, weights=w))
    assert np.array_equal(got["sd"], np.sqrt(np.full(5, 14.0) / 44)) and np.array_equal(got["p_above"], got["mean"] / 1e4)
    # a range that starts on a slab edge takes nothing along
    b = _Recorder()
    fit2, _, _ = sc.fake_fit(0, n_chain=1, samplers=[b])
    by2 = np.r_[np.zeros(64, dtype=np.int64), np.ones(10, dtype=np.int64), np.full(6, 2)]
    fit2.predict_groups(by2, np.zeros((80, 3)), level_bytes=8 * 15 * 2)
    assert [(c["n_levels"], len(c["level"])) for c in b.calls] == [(1, 64), (1, 10), (2, 16)] and np.array_equal(b.calls[2]["level"], [0] * 10 + [1] * 6)
    apart = fit.predict_groups(by, x, return_draws=True, combine_chains=False, type="indiv.bart")
    assert apart["average"].shape == (5, 15, 3) and a.calls[-1]["dense"] is None and a.calls[-1]["offset"] is None
    # any arm-0 argument, or treatment=, makes it the contrast
    fit.predict_groups("g.1", x, X=X, groups=new_terms, treatment=("X", 1), statistic="sum")
    call = a.calls[-1]
    assert call["n_arms"] == 2 and call["statistic"] == "sum" and call["dense0"] is not None and call["x_test0"] is None
    assert np.all(call["dense"][:, 1] == 1.0 - fit.X_means[1]) and np.all(call["dense0"][:, 1] == 0.0 - fit.X_means[1])
    fit.predict_groups(by, x, x_bart0=x + 1.0)
    assert a.calls[-1]["n_arms"] == 2 and np.array_equal(a.calls[-1]["x_test0"], (x + 1.0)[order])
