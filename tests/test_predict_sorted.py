"""s4b_predict_sorted without a GPU: the numpy model of tests/sorted_cases.py against an independent brute force (sorted() with the key, Python loops
over every row and draw) on random values, on values rounded to one decimal so that ties abound, and on the planted matrices with their hand-written
values; the m rule of the top and bottom groups; every refusal of the argument checks, which run on every device layer before anything is launched;
the launch refusal of the emulated layer (no selection kernels there), of the test entry too; the entries' absence from the oracle library and their
presence in the header; the interface version.  The kernels are tested in tests/test_gpu_predict_sorted.py."""
import os
import re

import numpy as np
import pytest

import describe_cases as dc
import sorted_cases as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _against_brute_force(x, row_probs, cut_rank):
    ref, bf = so.model(x, row_probs, cut_rank), so.brute_force(x, row_probs, cut_rank)
    assert so.same_bits(ref["sorted"], np.array(bf["sorted"]).reshape(ref["sorted"].shape))
    assert so.same_bits(ref["cut"], np.array(bf["cut"]).reshape(ref["cut"].shape))
    assert np.array_equal(ref["n_above"], np.array(bf["n_above"]).reshape(ref["n_above"].shape))
    assert np.array_equal(ref["n_below"], np.array(bf["n_below"]).reshape(ref["n_below"].shape))


@pytest.mark.parametrize("n", [1, 2, 7, 64, 101])
def test_model_against_a_brute_force_loop(n):
    g = np.random.default_rng(n)
    probs = (0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0, 1.0 / 3.0)
    ranks = sorted({0, n - 1, n // 2, max(0, n // 2 - 1), (9 * n) // 10})
    _against_brute_force(g.normal(size=(n, 6)), probs, ranks)
    tied = np.round(g.normal(size=(n, 6)), 1) + 0.0          # one decimal: ties abound, at the ranks too
    tied[::3] = -np.abs(tied[::3])                           # (-0.0 among them)
    _against_brute_force(tied, probs, ranks)
    if n >= 64:
        y = so.sorted_columns(tied)
        assert np.any(y[n // 2] == y[n // 2 - 1]), "the rounded columns hold no tie at the middle rank: the case does not test what it says"
        assert np.any(np.signbit(tied) & (tied == 0.0))


def test_key_order_and_its_inverse():
    v = np.array([-np.inf, -1.7976931348623157e308, -1.0, -5e-324, -0.0, 0.0, 5e-324, 2.2250738585072014e-308, 1.0, 1.7976931348623157e308, np.inf])
    k = so.key(v)
    assert np.all(k[1:] > k[:-1]) and so.same_bits(so.value(k), v)
    assert [so._py_key(float(x)) for x in v] == [int(x) for x in k]


def test_model_and_brute_force_on_the_planted_matrices():
    for name, p in so.PLANTED.items():
        x = np.array(p["x"])
        for got in (so.model(x, (), p["ranks"]), so.brute_force(x, (), p["ranks"])):
            assert so.same_bits(np.array(got["cut"]), np.array(p["order_stats"])), name
        for got in (so.model(x, (), p["cut_rank"]), so.brute_force(x, (), p["cut_rank"])):
            assert np.array_equal(np.array(got["n_above"]), np.array(p["n_above"])) and np.array_equal(np.array(got["n_below"]), np.array(p["n_below"])), name
    # type 7 across the rows: n = 101 at 0.5 is the order statistic of rank 50 itself; n = 4 at 0.5 is halfway between ranks 1 and 2
    assert so.type7_rows(0.5, 101) == (50, 51, 0.0) and so.type7_rows(0.5, 4) == (1, 2, 0.5)
    assert so.type7_rows(0.0, 9) == (0, 1, 0.0) and so.type7_rows(1.0, 9) == (8, 8, 0.0) and so.type7_rows(0.5, 1) == (0, 0, 0.0)
    assert so.targets(101, (0.5, 0.0, 1.0), (50, 7)) == [0, 7, 50, 100] and so.targets(4, (0.5,), ()) == [1, 2]


def test_m_rule_of_the_groups():
    from stan4bart_amd.abi import fraction_count
    for f, n, m in ((0.1, 1000, 100), (0.07, 100, 7), (0.1, 60, 6), (0.1, 61, 7), (0.5, 3, 2), (0.999, 1000, 999), (1e-9, 13, 1), (0.3, 10, 3)):
        assert fraction_count(f, n) == m == so.fraction_count(f, n), (f, n)
    assert int(np.ceil(0.07 * 100)) == 8          # what floating point gives: 0.07 x 100 is 7.000000000000001
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match=r"must lie in \(0, 1\)"):
            fraction_count(bad, 10)
    with pytest.raises(ValueError, match="is all of them"):
        fraction_count(0.95, 10)
    assert so.group_ranks(100, top=(0.07,), bottom=(0.07, 0.5)) == [92, 7, 50]
    # without ties at the boundary exactly m rows are in the group in every draw
    x = np.random.default_rng(3).permuted(np.tile(np.arange(100.0)[:, None], (1, 5)), axis=0)
    ref = so.model(x, (), so.group_ranks(100, top=(0.07,), bottom=(0.07,)))
    assert np.all((x > ref["cut"][0][None, :]).sum(axis=0) == 7) and np.all((x < ref["cut"][1][None, :]).sum(axis=0) == 7)
    assert ref["n_above"][0].sum() == 7 * 5 and ref["n_below"][1].sum() == 7 * 5


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
        assert smp.sorted_draws() == S

        def refused(match, **kw):
            args = dict(x_test=x, row_probs=(0.5,), cut_rank=(3,), probs=(0.5,))
            args.update(kw)
            with pytest.raises(RuntimeError, match=match):
                smp.predict_sorted(**args)
            assert not any(smp.sorted_info.values()), smp.sorted_info

        refused(r"predict_sorted: n_row_probs must lie in \[0, 12\], not 13", row_probs=np.linspace(0, 1, 13))
        refused(r"predict_sorted: n_cuts must lie in \[0, 8\], not 9", cut_rank=[1] * 9)
        refused(r"predict_sorted: row prob 1.5\d* outside \[0, 1\]", row_probs=(0.5, 1.5))
        refused(r"predict_sorted: row prob -0.1\d* outside \[0, 1\]", row_probs=(-0.1,))
        refused(r"predict_sorted: row prob nan outside \[0, 1\]", row_probs=(np.nan,))
        refused(r"predict_sorted: cut_rank 7 outside \[0, 6\]", cut_rank=(0, 7))
        refused(r"predict_sorted: cut_rank -1 outside \[0, 6\]", cut_rank=(-1,))
        refused("between 0 and 16 probs per call, not 17", probs=np.linspace(0, 1, 17))
        refused(r"prob 1.5\d* outside \[0, 1\]", probs=(0.5, 1.5))
        refused("predict_sorted: n_arms must be 1 .* or 2 .*, not 0", n_arms=0)
        refused("predict_sorted: n_arms must be 1 .* or 2 .*, not 3", n_arms=3)
        refused("predict_sorted: n_arms = 1 takes no arm-0 pointer", x_test0=x)
        refused("predict_sorted: n_arms = 1 takes no arm-0 pointer", offset=np.zeros(7), offset0=np.zeros(7))
        refused("predict_sorted: arms.rows.n_weights must be 0", weights=np.ones(7))
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
        refused("pooled draws, at most 16384", peers=[ch.stored[13]] * 1300)
        # the same refusals hold for the query form (every output NULL): the checks run before the plan is formed
        refused(r"predict_sorted: cut_rank 7 outside \[0, 6\]", cut_rank=(7,), outputs=())
        refused(r"predict_sorted: row prob 2.0\d* outside", row_probs=(2.0,), outputs=())
        assert np.array_equal(ch.live.get_counters(), before)
        with pytest.raises(ValueError, match="outputs must be among"):
            smp.predict_sorted(x, outputs=("median",))
        with pytest.raises(ValueError, match="cut_rank must be a vector of integers"):
            smp.predict_sorted(x, cut_rank=(0.5,))
        with pytest.raises(ValueError, match=r"must lie in \(0, 1\)"):
            smp.predict_sorted(x, top=(1.0,))
        with pytest.raises(ValueError, match="is all of them"):
            smp.predict_sorted(x, bottom=(0.9,))


def test_an_output_whose_count_is_zero_is_refused(emul_lib, chain):
    """The binding leaves such an output out, so the entry is called as a C caller would call it."""
    import ctypes as C
    from stan4bart_amd import abi
    ch = chain
    smp = ch.live
    x = np.asfortranarray(ch.x[:7])
    arms, keep, rows, _, S, pr = smp._contrast_in(lambda s: s.sorted_draws(), x, None, (), (), None, None, None, None, None, None, None, None, None, None, None, None, 0,
                                                  None, "auto", 0, 0)
    buf, cnt = np.zeros(64), np.zeros(64, dtype=np.int32)
    rp, ct = np.array([0.5]), np.array([3], dtype=np.int32)
    fn = smp._f("predict_sorted")

    def call(n_row_probs, n_cuts, **outs):
        arg = abi.SortedIn(arms=arms, n_arms=1, n_row_probs=n_row_probs, row_probs=abi._dp(rp), n_cuts=n_cuts, cut_rank=abi._ip(ct))
        out = abi.SortedOut(**outs)
        rc = fn(smp._h, C.byref(arg), C.byref(out))
        assert rc != 0 and not any(out.info)
        return smp._f("last_error")().decode()
    assert "but n_row_probs + n_cuts = 0" in call(0, 0, mean=abi._dp(buf))
    assert "but n_row_probs + n_cuts = 0" in call(0, 0, draws=abi._dp(buf))
    assert "quantiles given, but n_probs = 0" in call(1, 0, quantiles=abi._dp(buf))
    assert "n_above or n_below given, but n_cuts = 0" in call(1, 0, n_above=abi._ip(cnt))
    assert "n_above or n_below given, but n_cuts = 0" in call(1, 0, n_below=abi._ip(cnt))
    assert "no selection kernels" in call(1, 1, mean=abi._dp(buf))          # (a valid call: the emulated layer's refusal)
    del keep


def test_launch_is_refused_on_the_emulated_layer(emul_lib, chain):
    assert hasattr(emul_lib, "emu_predict_sorted") and hasattr(emul_lib, "emu_test_sorted_select")
    ch = chain
    x = ch.x[:7]
    col = ch.used_column(13)
    for smp in (ch.live, ch.stored[5]):
        before = ch.live.get_counters()
        with pytest.raises(RuntimeError, match="predict_sorted: this device layer has no selection kernels"):
            smp.predict_sorted(x, row_probs=(0.1, 0.5), top=(0.2,), bottom=(0.2,), probs=(0.025, 0.975))
        with pytest.raises(RuntimeError, match="no selection kernels"):
            smp.predict_sorted(x, ch.arm0(col)[:7], n_arms=2, cut_rank=(2,), outputs=("n_above",), peers=[ch.stored[1], ch.stored[2]])
        with pytest.raises(RuntimeError, match="no selection kernels"):          # the query for the plan is the device layer's too
            smp.predict_sorted(x, row_probs=(0.5,), outputs=())
        assert not any(smp.sorted_info.values()) and np.array_equal(ch.live.get_counters(), before)
        with pytest.raises(RuntimeError, match="no describe kernel"):          # the sibling's refusal is what it was
            smp.predict_describe(x, hdi_count=(3,))
        # the test entry: its checks run, the launch is refused
        v = np.arange(12.0).reshape(4, 3)
        with pytest.raises(RuntimeError, match="test_sorted_select: this device layer has no selection kernels"):
            smp.test_sorted_select(v, 8, ranks=(0, 3))
        for match, kw in ((r"rank 4 outside \[0, 3\]", dict(ranks=(4,))), ("neither ranks nor cuts", {}), (r"n_cuts must lie in \[0, 8\]", dict(cut_rank=[0] * 9)),
                          (r"n_ranks must lie in \[0, 32\]", dict(ranks=[0] * 33)), ("block_draws must be at least 1", dict(ranks=(0,), block_draws=0))):
            with pytest.raises(RuntimeError, match="test_sorted_select: " + match):
                smp.test_sorted_select(v, kw.pop("block_draws", 8), **kw)
        with pytest.raises(RuntimeError, match="more than 32 distinct ranks"):
            smp.test_sorted_select(np.zeros((40, 2)), 8, ranks=np.arange(32), cut_rank=(32,))
        with pytest.raises(RuntimeError, match="not finite"):
            smp.test_sorted_select(np.array([[0.0, np.inf]]), 8, ranks=(0,))


def test_oracle_library_has_no_entry_and_the_header_has_it(oracle_lib):
    from stan4bart_amd.abi import Sampler
    assert not hasattr(oracle_lib, "orc_predict_sorted") and not hasattr(oracle_lib, "orc_test_sorted_select")
    s = Sampler.__new__(Sampler)
    s._lib, s._pfx = oracle_lib, "orc_"
    with pytest.raises(RuntimeError, match="no predict_sorted"):
        Sampler.predict_sorted(s, np.zeros((2, 3)))
    header = open(os.path.join(ROOT, "include", "stan4bart_amd.h")).read()
    assert re.search(r"int S4B_FN\(predict_sorted\)\(s4b_sampler\* s, const s4b_sorted_in\* in, s4b_sorted_out\* out\);", header)
    assert re.search(r"int S4B_FN\(test_sorted_select\)\(s4b_sampler\* s, const double\* values, int64_t n, int64_t S, int64_t block_draws,", header)
    for said in ("-0.0 stands before +0.0", "R's type 7 ACROSS THE ROWS", "the order statistic itself, bit for bit", "both strict, both in DOUBLE comparison",
                 "counts on neither side", "depends on nothing but the multisets of the columns", "S4B_SORTED_PROBS_MAX 12", "S4B_SORTED_CUTS_MAX 8",
                 "n_test >= 2^31", "s4b_contrast_in arms;", "return the same bits", "Another order of the peers permutes the columns of D"):
        assert said in header, said


def test_interface_version_is_unchanged():
    header = open(os.path.join(ROOT, "include", "stan4bart_amd.h")).read()
    assert re.search(r"^#define S4B_INTERFACE_VERSION 6$", header, re.M)
    from stan4bart_amd import abi
    assert abi.INTERFACE_VERSION == 6
    assert [f[0] for f in abi.SortedIn._fields_] == ["arms", "n_arms", "n_row_probs", "row_probs", "n_cuts", "cut_rank"]
    assert [f[0] for f in abi.SortedOut._fields_] == ["mean", "m2", "quantiles", "draws", "n_above", "n_below", "num_samples", "info"]
    assert abi.SORTED_PROBS_MAX == so.PROBS_MAX and abi.SORTED_CUTS_MAX == so.CUTS_MAX


def test_fit_method_checks_its_arguments():
    import summary_cases as sc
    fit, _, _ = sc.fake_fit(0)
    with pytest.raises(ValueError, match="requires 'bart_args' to contain 'keepTrees'"):
        fit.predict_sorted(np.zeros((3, 2)))
    fit.samplers = [object()]
    xb = np.random.default_rng(0).normal(size=(30, 3))
    with pytest.raises(ValueError, match="does not form 'ppd'"):
        fit.predict_sorted(xb, type="ppd")
    with pytest.raises(ValueError, match="'row_probs' must be a vector of at most 12"):
        fit.predict_sorted(xb, row_probs=np.linspace(0, 1, 13))
    with pytest.raises(ValueError, match="'row_probs' must be a vector of at most 12"):
        fit.predict_sorted(xb, row_probs=(1.5,))
    with pytest.raises(ValueError, match="at most 8 per call"):
        fit.predict_sorted(xb, top=np.linspace(0.1, 0.5, 5), bottom=np.linspace(0.1, 0.4, 4))
    with pytest.raises(ValueError, match=r"must lie in \(0, 1\)"):
        fit.predict_sorted(xb, top=(0.0,))
    with pytest.raises(ValueError, match="is all of them"):
        fit.predict_sorted(xb, bottom=(0.99,))
