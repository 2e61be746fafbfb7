"""CPU twin of tests/test_gpu_readout.py: the same case builders (tests/readout_cases.py) at the same branch-selecting values over the emulated device
layer, whose predict_stored, test-fit and count loops are plain C++.  Nothing here says anything about the HIP kernels; what is pinned where no GPU
exists: the reference walk and its bound, the host's binning of new rows (SamplerCore::bin_matrix, single-threaded and on its thread pool) against the
rule "go left iff x <= cut value", the packing of the kept trees, exported states, the case builders, and — from the constants READ from dev_hip.hip —
which kernel and branch every named case is FOR, so that the GPU module's cases cannot drift away from their branches without a failure in this suite.
No size is shrunk: every branch here is selected by the number of test rows, trees or predictors, and those cost the emulation little."""
import numpy as np
import pytest

import readout_cases as rc


def test_limits_are_the_ones_the_cases_were_written_for():
    """The thresholds as the cases assume them; the tables of expected branches below are checked case by case."""
    L = rc.readout_limits()
    assert L == dict(block=256, grid_max=2048, tf_rows=4, few_rows=65536, few_lds=48 * 1024, predict_grid=4096, draw_k_block=256, bin_threads_from=1 << 22), L


@pytest.mark.parametrize("name", sorted(rc.TEST_FIT_CASES))
def test_test_fit_case_selects_the_branch_it_is_named_for(name):
    _, n_test, T = rc.TEST_FIT_CASES[name]
    rc.check_test_fit_branch(name, n_test, T)


@pytest.mark.parametrize("name", sorted(rc.PREDICT_CASES))
def test_predict_case_selects_the_branch_it_is_named_for(name):
    build, rows, draws = rc.PREDICT_CASES[name]
    P = {"c5-200x140": 140, "deep": 10}.get(name, 9)
    br = rc.predict_branch(max(rows, 1), draws, P)
    assert (br["rounds"], br["threaded_binning"]) == rc.PREDICT_EXPECTED[name], br
    L = rc.readout_limits()
    cap = L["predict_grid"] * L["block"]
    if name == "cap-exact":
        assert rows * draws == cap
    if name == "cap-plus-1":
        assert rows * draws == cap + 1
    if name == "three-caps":
        assert rows % 2 == 1 and draws > 1 and 3 * cap < rows * draws < 3 * cap + 64
    if name == "threaded-binning":
        assert P * rows >= L["bin_threads_from"] > P * (rows - 40000)


@pytest.mark.parametrize("name", sorted(rc.COUNT_CASES))
def test_count_case_selects_the_loops_it_is_named_for(name):
    _, P, T = rc.COUNT_CASES[name]
    br = rc.counts_branch(P, T)
    assert (br["p_rounds"], br["t_rounds"]) == rc.COUNT_EXPECTED[name], br


def test_walk_on_a_hand_made_tree():
    """The reference itself on two draws of two trees written out by hand: preorder, raw cut values, `<=` goes left."""
    trees = dict(sample=np.array([0, 0, 0, 0, 0, 0, 1, 1, 1, 1], dtype=np.int32), tree=np.array([0, 0, 0, 0, 0, 1, 0, 1, 1, 1], dtype=np.int32),
                 var=np.array([0, 1, -1, -1, -1, -1, -1, 1, -1, -1], dtype=np.int32),
                 value=np.array([0.5, 2.0, 0.125, 0.25, -0.5, 0.0625, 1.0, -1.0, 0.5, 0.25]))
    x = np.array([[0.5, 2.0], [0.5, np.nextafter(2.0, 3.0)], [np.nextafter(0.5, 1.0), -np.inf], [-np.inf, np.inf]])
    f, bound = rc.walk_fits(trees, x, [[10.0, 14.0], [0.0, 2.0]])
    inner = np.array([[0.125 + 0.0625, 1.25], [0.25 + 0.0625, 1.25], [-0.5 + 0.0625, 1.5], [0.25 + 0.0625, 1.25]])
    assert np.array_equal(f, (inner + 0.5) * np.array([4.0, 2.0]) + np.array([10.0, 0.0]))
    assert np.all(bound > 0) and np.all(bound < 1e-13)
    fb, _ = rc.walk_fits(trees, x, [0.0, 1.0], binary=True)
    assert np.array_equal(fb, inner)
    assert np.array_equal(rc.nodes_per_tree(trees), [5, 1, 1, 3])
    assert np.array_equal(rc.count_rules(trees, 2, 2), [[1, 0], [1, 1]])


def _report(line):
    print(line)


@pytest.mark.parametrize("name", sorted(rc.PREDICT_CASES))
def test_predictions(emul_lib, name):
    rc.assert_prediction_case(name, rc.check_prediction(emul_lib, "emu_", name, _report))


def test_per_draw_scale(emul_lib):
    rc.check_per_draw_scale(emul_lib, "emu_", _report)


@pytest.mark.parametrize("name", sorted(rc.TEST_FIT_CASES))
def test_test_row_fits(oracle_lib, emul_lib, name):
    rc.check_test_fits(emul_lib, "emu_", oracle_lib, name, _report)


@pytest.mark.parametrize("name", sorted(rc.COUNT_CASES))
def test_var_counts_and_k(oracle_lib, emul_lib, name):
    r = rc.check_counts(emul_lib, "emu_", oracle_lib, name, _report)
    if name == "predictors-299":
        assert np.flatnonzero(r["varcount"].sum(axis=1)).max() >= 256          # rules on predictors beyond the first round of the clearing loop were accepted


def test_more_predictors_than_a_rule_can_name_are_refused(emul_lib):
    rc.check_predictor_limit(emul_lib, "emu_")
