"""The fixed-point O(N) sums of the Stan block ALONE on the GPU (k_stan_fused + k_stan_forward + fetch_fused / recentre_scales and the plain-double
pipeline behind them), one evaluation at a time through s4b_test_stan_sums, against the references of tests/stan_sum_cases.py: exact data come back
bit for bit whenever the evaluation is accepted (and as the exact sums when it is not), the verdict, the magnitude and exponent words and the grid
equal what the data imply, random data stay within 4 x the derived bound on the path the evaluation took.  The path of every evaluation is asserted
from the entry's info.  tests/test_stan_sums.py is the CPU twin (the same cases over the emulation; it pins the references, the constants, the branch of
every case and the derived verdicts)."""
import numpy as np
import pytest

import stan_sum_cases as S

pytestmark = pytest.mark.gpu

RATIOS = {}


def _note(group, rep):
    g = RATIOS.setdefault(group, {})
    for k, v in rep.items():
        g[k] = max(g.get(k, 0.0), v)


@pytest.mark.parametrize("name", sorted(S.geometry_cases()))
def test_geometry_cases_are_exact(hip_lib, name):
    """Case a: every n at the edges of the launch geometry, every instantiation and branch a shape selects, weighted and not; mode 0 and DIRECT."""
    out = S.run_geometry_case(hip_lib, "s4b_", name)
    assert out["paths"] == ["fused", "fused"], out
    assert all(i["grid"] == out["branch"]["grid"] for i in out["info"])
    if name == "n-grid-cap":
        assert out["branch"]["grid"] == S.limits()["grid_cap"]


@pytest.mark.parametrize("t", [2.0 ** -50, -2.0 ** -50, 0.0], ids=["plus", "minus", "zero"])
@pytest.mark.parametrize("order", [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)], ids=lambda o: "".join(map(str, o)))
def test_cancellation_across_workgroups_is_exact(hip_lib, order, t):
    """Case b: +2^21, -2^21 and t in three workgroups (X'e), in two waves of one workgroup and a second workgroup (Z'e), in every order."""
    assert S.run_cancellation(hip_lib, "s4b_", order, t) == "fused"


def test_determinism_and_buffer_hygiene(hip_lib):
    """Case c: repeated evaluations are bit-identical; after an evaluation rejected for range or for resolution the next ones are exact again."""
    paths, kinds = S.run_hygiene(hip_lib, "s4b_")
    assert paths == ["fused" if k == "good" else "plain" for k in kinds], list(zip(kinds, paths))


@pytest.mark.parametrize("n,K,terms", [(300, 17, [(4, 0)]), (4200, 2, [(4097, 0)])], ids=["K17", "q4097"])
def test_shapes_without_the_fixed_point_path(hip_lib, n, K, terms):
    S.run_plain_shape(hip_lib, "s4b_", n, K, terms)


@pytest.mark.parametrize("name", sorted(S.edge_cases()))
def test_the_three_checks_at_their_edges(hip_lib, name):
    """Case d: the verdict of every point is derived from the data (the CPU twin pins the derivation), the sums are exact on either side."""
    S.run_edges(hip_lib, "s4b_", name)


@pytest.mark.parametrize("cancelling", [False, True], ids=["one-sign", "cancelling"])
@pytest.mark.parametrize("s_exp", [-200, -60, 0, 45, 60, 200])
def test_adaptation_reaches_the_fixed_point_path_and_stays(hip_lib, s_exp, cancelling):
    """Case e."""
    first, budget = S.run_adaptation(hip_lib, "s4b_", s_exp, cancelling)
    print(f"scale 2^{s_exp}{' cancelling' if cancelling else ''}: first accepted evaluation {first}, allowed {budget}")


def test_input_beyond_the_clamp_always_falls_back(hip_lib):
    S.run_adaptation(hip_lib, "s4b_", S.BEYOND_CLAMP, False, beyond_clamp=True)


@pytest.mark.parametrize("name", ["n257", "K16", "z5", "z-ragged", "q513", "params-65", "n-33-workgroups"])
def test_random_data_within_the_bound(hip_lib, name):
    rep = {}
    paths = S.run_bounded(hip_lib, "s4b_", name, rep)
    _note("random data", rep)
    print(f"{name}: paths {paths}, ratios to the bounds {rep}")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("binary", [False, True], ids=["continuous", "binary"])
def test_direct_against_indirect(hip_lib, binary, mode):
    """Case f."""
    from conftest import binary_case
    from large_cases import stan_shape_case
    args = binary_case(n=300, T=5, warmup=3, iter=6) if binary else stan_shape_case(300, 3, [(5, 1)], 7800, 1, weights=True, iters=(3, 6), trees=4, plain_init=True)
    rep = {}
    S.run_direct_against_indirect(hip_lib, "s4b_", args, mode, rep)
    _note("direct against indirect", rep)


@pytest.mark.parametrize("bad", [np.inf, np.nan], ids=["inf", "nan"])
def test_non_finite_coefficients(hip_lib, bad):
    """Case g."""
    S.run_non_finite(hip_lib, "s4b_", bad)


def test_the_entry_leaves_a_run_alone(hip_lib):
    """Two samplers, one of which answers a handful of test evaluations (with exponents far off) between create and run: the chains are bit-identical."""
    from conftest import friedman_case, make_sampler
    out = []
    for probe in (False, True):
        args, _ = friedman_case(n=300, T=5, warmup=4, iter=8, stan_args={"hmc_mode": 1})
        s = make_sampler(hip_lib, "s4b_", args)
        try:
            if probe:
                for ex in ((200, -300, 50), None, None):
                    s.test_stan_sums(1, set_exp=ex)
                    s.test_stan_sums(-1, np.zeros(s.K), np.zeros(s.q))
                s.test_stan_sums(1)                                  # (e0 as run() left it: the sampler's own mode)
            out.append(s.run(4, True)["stan"])
        finally:
            s.free()
    S.same_bits(out[0], out[1], "a run after test evaluations")


def test_the_entry_is_refused_on_a_stored_sampler(hip_lib):
    from conftest import friedman_case, make_sampler
    from stan4bart_amd.abi import Sampler, StoredSampler
    args, _ = friedman_case(n=80, T=3, warmup=2, iter=4)
    args.keep_trees = True
    s = make_sampler(hip_lib, "s4b_", args)
    try:
        s.run(2, True)
        s.disengage_adaptation()
        s.run(2, False)
        stored = StoredSampler(hip_lib, "s4b_", s.export_bart_state())
        try:
            stored.K, stored.q = s.K, s.q
            with pytest.raises(RuntimeError, match="live sampler"):
                Sampler.test_stan_sums(stored, 0)
        finally:
            stored.free()
    finally:
        s.free()


@pytest.fixture(scope="module", autouse=True)
def report_the_largest_ratios():
    """Not a check and not a test: when the module is through, prints (under -s) the largest observed ratio to each derived bound, per group of the
    cases that ran.  The asserted bounds stay the derived ones."""
    yield
    for group in sorted(RATIOS):
        print(f"largest ratios, {group}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(RATIOS[group].items())))
