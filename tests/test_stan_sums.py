"""CPU twin of tests/test_gpu_stan_sums.py: the same cases (tests/stan_sum_cases.py) through the test entry s4b_test_stan_sums over the emulated device
layer, which evaluates in plain doubles and serial order.  What this file pins is the references and the bounds themselves — an exact case must come
back as the exact sums rounded once, a bounded case within the bound with the serial depth — the constants read from the source, the shape -> branch
expectations of every case (a table written by hand), the verdicts the edge cases derive, and the refusals of the entry."""
import numpy as np
import pytest

import stan_sum_cases as S

RATIOS = {}


def _note(group, rep):
    g = RATIOS.setdefault(group, {})
    for k, v in rep.items():
        g[k] = max(g.get(k, 0.0), v)


def test_the_constants_are_the_documented_ones():
    L = S.limits()
    assert (L["sblock"], L["copies"], L["grid_cap"], L["fx_limit"], L["word_bits"], L["ex_min"], L["target"], L["clamp"], L["step"], L["total_target"]) == \
        (256, 32, 2048, 2 ** 42, 32, 4, 22, 900, 10, 20)
    assert (L["qmax"], L["zmax"], L["inline"], L["chunk"]) == (4096, 4, 64, 4096)
    assert [S.fused_grid(n, L) for n in (1, 256, 257, 8193, 16384, 524545)] == [1, 1, 2, 33, 64, 2048]


# name -> (n, kmax, zfixed, ncopy, par_inline, workgroups): written by hand from the kernel's comments, not computed
BRANCHES = {
    "n1": (1, 2, 1, 4, True, 1), "n63": (63, 2, 2, 4, True, 1), "n64": (64, 2, 2, 4, True, 1), "n255": (255, 2, 2, 4, True, 1),
    "n256": (256, 2, 2, 4, True, 1), "n257": (257, 2, 2, 4, True, 2),
    "n-33-workgroups": (8193, 2, 1, 4, True, 33), "n-64-workgroups": (16384, 2, 2, 4, True, 64), "n-grid-cap": (524545, 2, 1, 4, True, 2048),
    "K1": (300, 2, 1, 4, True, 2), "K2": (300, 2, 1, 4, True, 2), "K3": (300, 4, 1, 4, True, 2), "K4": (300, 4, 1, 4, True, 2),
    "K5": (300, 8, 1, 4, True, 2), "K8": (300, 8, 1, 4, True, 2), "K9": (300, 16, 1, 4, True, 2), "K16": (300, 16, 1, 4, True, 2),
    "K0": (300, 2, 2, 4, True, 2), "q0": (300, 4, -1, 4, True, 2), "z0": (300, 2, 0, 4, True, 2), "z3": (300, 2, 3, 4, True, 2),
    "z4": (300, 2, 4, 4, True, 2), "z5": (400, 2, -1, 4, True, 2), "z-ragged": (400, 8, -1, 4, True, 2), "z-empty-rows": (400, 2, -1, 4, True, 2),
    "q512": (1100, 2, 1, 4, False, 5), "q513": (1100, 2, 1, 1, False, 5), "inline-64": (500, 16, 1, 4, True, 2), "params-65": (500, 16, 1, 4, False, 2),
}


def test_every_case_selects_the_branch_it_was_built_for():
    L = S.limits()
    G = S.geometry_cases(L)
    assert sorted(G) == sorted(BRANCHES)
    for name, spec in G.items():
        if spec["n"] > 20000:
            continue                                                 # (the large case is built once, in the test that runs it)
        args = S.shape_case(seed=1, **spec)
        br = S.expected_branch(spec, args, L)
        assert br["fused"]
        assert (len(args.y), br["kmax"], br["zfixed"], br["ncopy"], br["par_inline"], br["grid"]) == BRANCHES[name], name
        d = np.diff(np.asarray(args.u))
        if name == "z5":
            assert set(d.tolist()) == {5}
        if name == "z-ragged":
            assert d.min() < d.max() and d.min() >= 1
        if name == "z-empty-rows":
            assert d.min() == 0 and d[-1] == 0 and d.max() == 4
        if name == "z0":
            assert len(args.w) == 0 and sum(int(a) * int(c) for a, c in zip(args.p, args.l)) == 4


def test_limbs_and_rounding_of_the_model():
    """The integer model's own pieces against hand-computed values."""
    assert [S._rne_scale(p, -1) for p in (1, 3, 5, -1, -3, 2)] == [0, 2, 2, 0, -2, 1]          # ties to even
    assert S._limbs(1, 56) == (1 << 20, 0)                               # 1.0
    assert S._limbs(1, 6) == (0, 64)                                     # 2^-50
    assert S._limbs(3, -2) == (0, 1)                                     # 3 2^-58 -> 2^-56 (0.75 rounds to 1)
    assert S._limbs(1, -1) == (0, 0)                                     # 2^-57: a tie, to even
    assert S._limbs(-((1 << 42) - 1), 56 - 0)[0] == -((1 << 42) - 1) << 20
    hi, lo = S._limbs((1 << 30) + 1, 56 - 30)                            # 1 + 2^-30: hi holds 1, lo the rest
    assert (hi, lo) == (1 << 20, 1 << 26)
    assert S._to_float(3, -1) == 1.5 and S._ilogb(5, -3) == -1


@pytest.mark.parametrize("name", sorted(S.edge_cases()))
def test_the_edges_derive_the_documented_verdicts(emul_lib, name):
    seen = S.run_edges(emul_lib, "emu_", name)
    if name == "one-workgroup":
        by = {(g, E): (mag, exw) for g, E, mag, exw in seen}
        for g in range(3):
            assert by[(g, 11)][0][g] == 2 ** 32 - 1 and by[(g, 12)][0][g] >= 2 ** 32
            assert by[(g, -26)][1][g] == 4004 and by[(g, -27)][1][g] == 4003
    if name == "two-workgroups-below":
        assert all(mag[g] == 2 ** 32 - 1 for g, E, mag, exw in seen)
    if name == "two-workgroups-at":
        assert all(mag[g] == 2 ** 32 for g, E, mag, exw in seen)


@pytest.mark.parametrize("name", [n for n in sorted(BRANCHES) if n != "n-grid-cap"])
def test_geometry_cases_are_exact_in_plain_doubles(emul_lib, name):
    out = S.run_geometry_case(emul_lib, "emu_", name)
    assert out["paths"] == ["plain", "plain"]


def test_the_large_case_is_exact_in_plain_doubles(emul_lib):
    out = S.run_geometry_case(emul_lib, "emu_", "n-grid-cap")
    assert out["branch"]["grid"] == 2048 and out["paths"] == ["plain", "plain"]


@pytest.mark.parametrize("t", [2.0 ** -50, -2.0 ** -50, 0.0])
def test_cancellation_across_workgroups(emul_lib, t):
    for order in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
        assert S.run_cancellation(emul_lib, "emu_", order, t) == "plain"


def test_hygiene_sequence(emul_lib):
    paths, kinds = S.run_hygiene(emul_lib, "emu_")
    assert set(paths) == {"plain"} and kinds.count("high") == 3 and kinds.count("low") == 2


@pytest.mark.parametrize("n,K,terms", [(300, 17, [(4, 0)]), (4200, 2, [(4097, 0)])], ids=["K17", "q4097"])
def test_shapes_without_the_fixed_point_path(emul_lib, n, K, terms):
    S.run_plain_shape(emul_lib, "emu_", n, K, terms)


@pytest.mark.parametrize("cancelling", [False, True], ids=["one-sign", "cancelling"])
@pytest.mark.parametrize("s_exp", [-200, -60, 0, 45, 60, 200])
def test_scaled_inputs_are_exact(emul_lib, s_exp, cancelling):
    S.run_adaptation(emul_lib, "emu_", s_exp, cancelling)


def test_adaptation_budgets():
    L = S.limits()
    assert S.adaptation_budget(3, False, False, L) == 2
    assert S.adaptation_budget(400, True, False, L) == 4
    assert S.adaptation_budget(205, True, True, L) == 22 and S.adaptation_budget(21, True, True, L) == 4


def test_input_beyond_the_clamp(emul_lib):
    S.run_adaptation(emul_lib, "emu_", S.BEYOND_CLAMP, False, beyond_clamp=True)


@pytest.mark.parametrize("name", ["n257", "K16", "z5", "z-ragged", "q513", "params-65", "n-33-workgroups"])
def test_bounded_cases_stay_within_the_serial_bound(emul_lib, name):
    rep = {}
    assert set(S.run_bounded(emul_lib, "emu_", name, rep)) == {"serial"}
    _note("bounded", rep)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("binary", [False, True], ids=["continuous", "binary"])
def test_direct_against_indirect(emul_lib, binary, mode):
    from conftest import binary_case
    from large_cases import stan_shape_case
    args = binary_case(n=300, T=5, warmup=3, iter=6) if binary else stan_shape_case(300, 3, [(5, 1)], 7800, 1, weights=True, iters=(3, 6), trees=4, plain_init=True)
    rep = {}
    S.run_direct_against_indirect(emul_lib, "emu_", args, mode, rep)
    _note("direct against indirect", rep)


@pytest.mark.parametrize("bad", [np.inf, np.nan], ids=["inf", "nan"])
def test_non_finite_coefficients(emul_lib, bad):
    S.run_non_finite(emul_lib, "emu_", bad)


def test_refusals(emul_lib):
    from conftest import friedman_case, make_sampler
    from stan4bart_amd.abi import Sampler, StoredSampler
    args, _ = friedman_case(n=80, T=3, warmup=2, iter=4)
    args.keep_trees = True
    s = make_sampler(emul_lib, "emu_", args)
    try:
        K, q = s.K, s.q
        for mode in (-2, 4):
            with pytest.raises(RuntimeError, match="mode must be"):
                s.test_stan_sums(mode)
        for mode in (2, 3):
            with pytest.raises(RuntimeError, match="user's offset"):
                s.test_stan_sums(mode)
        for ex in ((901, 0, 0), (0, -901, 0)):
            with pytest.raises(RuntimeError, match="exponent outside"):
                s.test_stan_sums(0, set_exp=ex)
        with pytest.raises(ValueError):
            s.test_stan_sums(-1, np.zeros(K + 1), np.zeros(q))
        sums, info = s.test_stan_sums(0)
        assert sums.shape == (1 + K + q,) and not info["fused"]
        s.run(2, True)
        s.disengage_adaptation()
        s.run(2, False)
        stored = StoredSampler(emul_lib, "emu_", s.export_bart_state())
        try:
            stored.K, stored.q = K, q
            with pytest.raises(RuntimeError, match="live sampler"):
                Sampler.test_stan_sums(stored, 0)
        finally:
            stored.free()
    finally:
        s.free()


def test_a_user_offset_admits_modes_2_and_3(emul_lib):
    from conftest import friedman_case, make_sampler
    g = np.random.default_rng(5)
    args, _ = friedman_case(n=120, T=3, warmup=2, iter=4, offset=g.standard_normal(120))
    s = make_sampler(emul_lib, "emu_", args)
    try:
        data = S.Data(args)
        sums, _ = s.test_stan_sums(2)
        ref, bound = S.bounded_model(data, (data.y.astype(S.LD) - np.asarray(args.offset).astype(S.LD)), None, None, (0, 0, 0), "serial",
                                     de0=S.U * np.abs(data.y - np.asarray(args.offset)))
        S.check_bounded(sums, ref, bound, "mode 2", {})
        s.test_stan_sums(3)
    finally:
        s.free()


@pytest.fixture(scope="module", autouse=True)
def report_the_largest_ratios():
    """Not a check: prints (under -s) the largest observed ratio to each derived bound per group of cases.  The asserted bounds stay the derived ones."""
    yield
    for group in sorted(RATIOS):
        print(f"largest ratios, {group}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(RATIOS[group].items())))
