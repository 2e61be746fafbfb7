"""s4b_predict_describe without a GPU: the numpy model of tests/describe_cases.py against an independent brute force (Python loops over every window and
every draw, sorted()) on random rows, on rows rounded to one decimal so that ties abound, and on the planted series with their hand-written values; the
m rule of the Python binding; every refusal of the argument checks, which run on every device layer before anything is launched; the launch refusal of
the emulated layer (no describe kernel there); the entry's absence from the oracle library and its presence in the header; the interface version.  The
kernel is tested in tests/test_gpu_predict_describe.py."""
import os
import re

import numpy as np
import pytest

import describe_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _against_brute_force(x, counts, thresholds):
    ref = dc.model(x, counts, thresholds)
    for i, row in enumerate(x):
        bf = dc.brute_force(row, counts, thresholds)
        assert ref["median"][i] == bf["median"] and ref["mad"][i] == bf["mad"], i
        for c in range(len(counts)):
            assert (ref["hdi"][c, 0, i], ref["hdi"][c, 1, i]) == bf["hdi"][c] and ref["hdi_start"][c, i] == bf["hdi_start"][c], (i, c)
        assert list(ref["n_above"][:, i]) == bf["n_above"] and list(ref["n_below"][:, i]) == bf["n_below"], i


@pytest.mark.parametrize("S", [1, 2, 7, 8, 23, 64])
def test_model_against_a_brute_force_loop(S):
    g = np.random.default_rng(S)
    x = g.normal(size=(12, S))
    counts = sorted({1, -(-S // 2), -(-19 * S // 20), S})
    thresholds = (0.0, float(x[3, 0]), dc.midpoint(x) if S > 1 else 0.25, -np.inf, np.inf)
    _against_brute_force(x, counts, thresholds)
    tied = np.round(g.normal(size=(12, S)), 1) + 0.0          # one decimal: ties abound, among the widths too
    tied[5] = -np.abs(tied[5])
    _against_brute_force(tied, counts, (0.0, -0.0, 0.1, float(tied[2, 0])))
    if S >= 23:
        assert not dc.unique_minimum(tied, -(-S // 2)).all(), "the rounded rows hold no tie of widths: the case does not test what it says"


def test_model_and_brute_force_on_the_planted_series():
    for S, group in dc.PLANTED.items():
        for name, (series, _) in group["rows"].items():
            assert len(series) == S
            dc.assert_planted(dc.brute_force(series, group["counts"], group["thresholds"]), S, name)
            x = np.array([series[::-1], series])          # (the order of the draws does not matter)
            ref = dc.model(x, group["counts"], group["thresholds"])
            dc.assert_planted(ref, S, name, 0)
            dc.assert_planted(ref, S, name, 1)
    tie = dc.PLANTED[7]["rows"]["two windows of equal width"][0]
    assert not dc.unique_minimum(np.array([tie]), 3)[0] and dc.unique_minimum(np.array([tie]), 7)[0]


def test_m_rule():
    from stan4bart_amd.generics import Stan4bartFit
    for ci, S, m in ((0.7, 10, 7), (0.95, 100, 95), (0.9, 7, 7), (1.0, 13, 13), (1.0, 1, 1), (1e-9, 13, 1), (0.5, 9, 5), (0.95, 16384, 15565), (0.07, 100, 7)):
        assert Stan4bartFit.hdi_draws(ci, S) == m == dc.hdi_draws(ci, S), (ci, S)
    assert int(np.ceil(0.07 * 100)) == 8          # what floating point gives: 0.07 x 100 is 7.000000000000001
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="'ci' must hold masses in"):
            Stan4bartFit.hdi_draws(bad, 10)


_CHAINS = {}


@pytest.fixture(scope="module")
def chain(emul_lib):
    _CHAINS["c"] = dc.small_chain(emul_lib, "emu_")
    yield _CHAINS["c"]
    _CHAINS.pop("c").close()


def test_every_refusal_before_any_launch(emul_lib, chain):
    ch = chain
    x = ch.x[:7]
    for smp, S in ((ch.live, 13), (ch.stored[5], 5)):
        before = ch.live.get_counters()
        assert smp.describe_draws() == S

        def refused(match, **kw):
            args = dict(x_test=x, hdi_count=(1,), thresholds=(0.0,), probs=(0.5,))
            args.update(kw)
            with pytest.raises(RuntimeError, match=match):
                smp.predict_describe(**args)
            assert not any(smp.describe_info.values()), smp.describe_info

        refused("predict_describe: n_hdi must lie in \\[0, 8\\], not 9", hdi_count=[1] * 9)
        refused("predict_describe: n_thresholds must lie in \\[0, 32\\], not 33", thresholds=np.arange(33.0))
        refused("between 0 and 16 probs per call, not 17", probs=np.linspace(0, 1, 17))
        refused(r"prob 1.5\d* outside \[0, 1\]", probs=(0.5, 1.5))
        refused(rf"predict_describe: hdi_count 0 outside \[1, {S}\]", hdi_count=(1, 0))
        refused(rf"predict_describe: hdi_count {S + 1} outside \[1, {S}\]", hdi_count=(S + 1,))
        refused(r"predict_describe: hdi_count -3 outside", hdi_count=(-3,))
        refused("predict_describe: threshold 1 is a NaN", thresholds=(0.0, np.nan))
        refused("predict_describe: n_arms must be 1 .* or 2 .*, not 0", n_arms=0)
        refused("predict_describe: n_arms must be 1 .* or 2 .*, not 3", n_arms=3)
        refused("predict_describe: n_arms = 1 takes no arm-0 pointer", x_test0=x)
        refused("predict_describe: n_arms = 1 takes no arm-0 pointer", offset=np.zeros(7), offset0=np.zeros(7))
        refused("predict_describe: arms.rows.n_weights must be 0", weights=np.ones(7))
        # whatever predict_contrast refuses
        refused("negative scratch_bytes", scratch_bytes=-1)
        refused("link must be 0", link=2)
        refused("route must be 0", route=3)
        refused("offset0 given, but arm 1 has no offset", n_arms=2, offset0=np.zeros(7))
        refused("dense0 given, but arm 1 has no dense part", n_arms=2, dense0=np.ones((7, 1)))
        three = np.asfortranarray(x.copy())
        three[:, :3] += 10.0
        refused("the arms differ in 3 BART columns", n_arms=2, x_test0=three)
        refused("x_test0 holds a NaN", n_arms=2, x_test0=np.full_like(x, np.nan))
        refused(r"ell_index 5 outside \[-1, 2\)", ell_index=np.full((7, 1), 5), ell_value=np.ones((7, 1)), ell_coef=np.ones((S, 2)))
        refused("pooled draws, at most 16384", peers=[ch.stored[13]] * 1300)
        # the same refusals hold for the query form (every output NULL): the checks run before the plan is formed
        refused(rf"predict_describe: hdi_count {S + 1} outside \[1, {S}\]", hdi_count=(S + 1,), outputs=())
        refused("predict_describe: threshold 0 is a NaN", thresholds=(np.nan,), outputs=())
        assert np.array_equal(ch.live.get_counters(), before)
        with pytest.raises(ValueError, match="outputs must be among"):
            smp.predict_describe(x, outputs=("mean",))
        with pytest.raises(ValueError, match="hdi_count must be a vector of integers"):
            smp.predict_describe(x, hdi_count=(0.95,))
        with pytest.raises(ValueError, match="thresholds must be a vector"):
            smp.predict_describe(x, thresholds=np.zeros((2, 2)))


def test_launch_is_refused_on_the_emulated_layer(emul_lib, chain):
    assert hasattr(emul_lib, "emu_predict_describe")
    ch = chain
    x = ch.x[:7]
    col = ch.used_column(13)
    for smp in (ch.live, ch.stored[5]):
        before = ch.live.get_counters()
        with pytest.raises(RuntimeError, match="predict_describe: this device layer has no describe kernel"):
            smp.predict_describe(x, hdi_count=(3,), thresholds=(0.0, 1.0), probs=(0.025, 0.975))
        with pytest.raises(RuntimeError, match="no describe kernel"):
            smp.predict_describe(x, ch.arm0(col)[:7], n_arms=2, hdi_count=(2,), outputs=("hdi", "mad"), peers=[ch.stored[1], ch.stored[2]])
        with pytest.raises(RuntimeError, match="no describe kernel"):          # the query for the plan is the device layer's too
            smp.predict_describe(x, outputs=())
        assert not any(smp.describe_info.values()) and np.array_equal(ch.live.get_counters(), before)
        with pytest.raises(RuntimeError, match="no level kernels"):          # the sibling's refusal is what it was
            smp.predict_groups(x, np.zeros(7, dtype=np.int64), 1)


def test_oracle_library_has_no_entry_and_the_header_has_it(oracle_lib):
    from stan4bart_amd.abi import Sampler
    assert not hasattr(oracle_lib, "orc_predict_describe")
    s = Sampler.__new__(Sampler)
    s._lib, s._pfx = oracle_lib, "orc_"
    with pytest.raises(RuntimeError, match="no predict_describe"):
        Sampler.predict_describe(s, np.zeros((2, 3)))
    header = open(os.path.join(ROOT, "include", "stan4bart_amd.h")).read()
    assert re.search(r"int S4B_FN\(predict_describe\)\(s4b_sampler\* s, const s4b_describe_in\* in, s4b_describe_out\* out\);", header)
    for said in ("-0.0 stands before +0.0", "the smallest width wins, on an exact tie the LOWEST j", "one double subtraction", "both strict, both in DOUBLE comparison",
                 "NOT pinned against HDInterval::hdi", "the type-7 median of |x(k) - median[i]|", "S4B_DESCRIBE_HDI_MAX 8", "S4B_DESCRIBE_THRESHOLDS_MAX 32",
                 "hdi_start included", "s4b_contrast_in arms;"):
        assert said in header, said


def test_interface_version_is_unchanged():
    header = open(os.path.join(ROOT, "include", "stan4bart_amd.h")).read()
    assert re.search(r"^#define S4B_INTERFACE_VERSION 6$", header, re.M)
    from stan4bart_amd import abi
    assert [f[0] for f in abi.DescribeIn._fields_] == ["arms", "n_arms", "n_hdi", "hdi_count", "n_thresholds", "thresholds"]
    assert [f[0] for f in abi.DescribeOut._fields_] == ["quantiles", "median", "hdi", "hdi_start", "n_above", "n_below", "mad", "num_samples", "info"]
    assert abi.DESCRIBE_HDI_MAX == dc.HDI_MAX and abi.DESCRIBE_THRESHOLDS_MAX == dc.THRESHOLDS_MAX


def test_fit_method_checks_its_arguments():
    import summary_cases as sc
    fit, _, _ = sc.fake_fit(0)
    with pytest.raises(ValueError, match="requires 'bart_args' to contain 'keepTrees'"):
        fit.describe_posterior(np.zeros((3, 2)))
    fit.samplers = [object()]
    xb = np.random.default_rng(0).normal(size=(30, 3))
    with pytest.raises(ValueError, match="does not form 'ppd'"):
        fit.describe_posterior(xb, type="ppd")
    with pytest.raises(ValueError, match="at most 8 per call"):
        fit.describe_posterior(xb, ci=np.linspace(0.1, 0.9, 9))
    with pytest.raises(ValueError, match="'thresholds' must be a vector without NaN"):
        fit.describe_posterior(xb, thresholds=(0.0, np.nan))
    with pytest.raises(ValueError, match="'rope' must be None or"):
        fit.describe_posterior(xb, rope=(0.1, -0.1))
    with pytest.raises(ValueError, match="at most 29 per call"):
        fit.describe_posterior(xb, thresholds=np.arange(30.0), rope=(-0.1, 0.1))
