"""The fused (k_step) and two-kernel (k_tree + k_control + k_apply) tree updates against the oracle at the sizes where the automatic choice takes them.
Below N_SWEEP_MAX every sampler runs the persistent sweep, and there the per-tree kernels' per-thread loops hardly run: k_step's pass threads route
their first F_PF = 2 quads in the prefetched block, k_tree's threads own one quad each.  Here k_step's "remaining quads" loop (two requests in flight,
agent-scope reloads of the residual in later bin passes) and k_tree's software pipeline (two quads ahead, loop-carried accumulators, NBMAX bin passes
that re-read the residual the thread has just written) run in steady state.  Every case asserts the path it was written for: if the thresholds of
choose_path move, these tests fail instead of quietly testing another kernel.  Same bar as everywhere: tree-move trace, trees and generator state
bit-exact, floating-point state to rtol 1e-6 / atol 1e-9.

The size limits (stan4bart_amd/csrc/dev_hip.hip, creation of the device arrays; nQuads = ceil(n / 4)):
  * persistent sweep (sweepRegsOk_): nQuads <= (gridF - 1) * SW_PT * SW_PF = 255 pass workgroups * 256 pass threads * 4 quads, i.e.
    n <= 1 044 480.  (k_step's prefetched block covers the same n: 255 * F_PT = 512 threads * F_PF = 2 quads.)
  * fused (fusedAuto_): perThread = ceil(nQuads / (255 * 512)) <= 8, i.e. n <= 255 * 512 * 8 * 4 = 4 177 920; never with split.probs (fusedOk_).
  * two-kernel beyond, with k_tree's grid of min(1024, nQuads / 256) workgroups of 256 threads: at n = 1e7 a thread owns 9 or 10 quads.
Oracle halves on one CPU core (these data, the same calls): about 2 s at n = 1 044 481, 4 - 8 s at n = 2e6 and 4.2e6, 15 - 40 s at n = 1e7."""
import numpy as np
import pytest

from conftest import StateView, assert_chain_parity, assert_state_parity, make_sampler, run_chain
from large_cases import sized_case

pytestmark = pytest.mark.gpu

N_SWEEP_MAX = 255 * 256 * 4 * 4           # 1 044 480: the last n of the persistent sweep
N_FUSED_MAX = 255 * 512 * 8 * 4           # 4 177 920: the last n of the fused path (8 quads on the busiest pass thread)


def _parity(oracle_lib, hip_lib, args, path, stan=False):
    rt = 0 if stan else 1
    a = run_chain(oracle_lib, "orc_", args, results_type=rt)
    b = run_chain(hip_lib, "s4b_", args, results_type=rt)
    assert b["tree_path"] == ("auto", path), b["tree_path"]
    assert_chain_parity(a, b, stan=stan)
    assert (a["trace"][:, 1] == 1).sum() > 0, "no move was accepted: nothing was tested"
    assert b["sweep_stats"][0] == 0, b["sweep_stats"]          # (no persistent launch ran)
    return a, b


def _max_nodes(trees):
    return int(np.bincount(trees["tree"]).max())


# ---- the fused path at its two boundaries and inside -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,trees", [(N_SWEEP_MAX + 1, 8), (N_FUSED_MAX, 6)], ids=["first-fused", "last-fused"])
def test_fused_at_its_boundaries(oracle_lib, hip_lib, n, trees):
    """n = 1 044 481: one quad (one observation) past the prefetched block, the remainder loop runs once on one thread.
    n = 4 177 920: 8 quads on the busiest pass thread, 6 of them in the remainder loop."""
    _parity(oracle_lib, hip_lib, sized_case(n, seed=1, trees=trees, iters=(2, 8)), "fused")


def test_two_kernel_at_its_boundary(oracle_lib, hip_lib):
    """n = 4 177 921: the first size beyond the fused path."""
    _parity(oracle_lib, hip_lib, sized_case(N_FUSED_MAX + 1, seed=2, trees=6, iters=(2, 8)), "two-kernel")


@pytest.mark.parametrize("kind", ["plain", "deep", "weighted", "k_chi"])
def test_fused_at_two_million(oracle_lib, hip_lib, kind):
    """4 quads per pass thread.  deep: more than 8 bins per proposal (several bin passes in one launch, the later ones reading back the residual the
    first stored) and more than 64 node slots (the global-memory control code of the last finishing workgroup).  weighted: k_step<weighted>.
    k_chi: a modeled k (k_chi)."""
    kw = dict(plain=dict(trees=10), deep=dict(trees=6, deep=True), weighted=dict(trees=8, weights=True),
              k_chi=dict(trees=8, k_chi=(1.25, float("inf"))))[kind]
    a, b = _parity(oracle_lib, hip_lib, sized_case(2_000_000, seed=3, iters=(2, 8), **kw), "fused")
    if kind == "deep":
        assert _max_nodes(a["trees"]) > 64, _max_nodes(a["trees"])
    if kind == "k_chi":
        assert "k" in b["sample"]["bart"]


def test_split_probs_at_two_million_take_the_two_kernel_path(oracle_lib, hip_lib):
    """cgm(split.probs = ): the fused path's wave-register control code has no weighted predictor choice (fusedOk_ is false), so at a size of the fused
    path the automatic choice is the two-kernel path."""
    _parity(oracle_lib, hip_lib, sized_case(2_000_000, seed=4, trees=8, iters=(2, 8), split_probs=True), "two-kernel")


# ---- the two-kernel path at n = 1e7 (BASELINE config 5's size, north_star's roofline target) --------------------------------------------------------

@pytest.mark.parametrize("kind", ["plain", "weighted", "deep"])
def test_two_kernel_at_ten_million(oracle_lib, hip_lib, kind):
    """9 - 10 quads per k_tree thread.  weighted: k_tree<., true> (8 bins per pass).  deep: more than NBMAX = 16 bins per proposal (several NBMAX passes)."""
    kw = dict(plain=dict(trees=8), weighted=dict(trees=8, weights=True), deep=dict(trees=6, deep=True))[kind]
    a, _ = _parity(oracle_lib, hip_lib, sized_case(10_000_000, seed=5, iters=(1, 4), **kw), "two-kernel")
    if kind == "deep":
        assert _max_nodes(a["trees"]) > 64, _max_nodes(a["trees"])


def test_joint_chain_at_ten_million(oracle_lib, hip_lib):
    """BART and the Stan block (a fixed effect, a random intercept of 5 groups, hmc_mode 0): the fixed-point O(N) Stan sums at N = 1e7."""
    args = sized_case(10_000_000, seed=6, trees=8, iters=(1, 3), joint=True, stan_args={"hmc_mode": 0})
    _, b = _parity(oracle_lib, hip_lib, args, "two-kernel", stan=True)
    assert b["fused_stats"][0] > 0, b["fused_stats"]


def test_stationary_two_kernel_at_ten_million_teacher_forced(oracle_lib, hip_lib):
    """The regime that is benchmarked, on the two-kernel path: 50 trees, the HIP chain burned in for 300 sweeps, adaptation disengaged, then the state
    injected into the oracle, both advance one iteration and everything is compared (trace, generator, fits, the whole state after the iteration), twice.
    Most moves are rejected here, so k_control's speculation on image 0 (the proposal made as if the previous one were rejected) mostly holds."""
    burn, T = 300, 50
    args = sized_case(10_000_000, seed=7, trees=T, iters=(burn, burn + 2), keep_fits=False)
    sp, so = make_sampler(hip_lib, "s4b_", args), make_sampler(oracle_lib, "orc_", args)
    try:
        sp.run(burn, True, 1)
        sp.disengage_adaptation(); so.disengage_adaptation()
        assert sp.get_tree_path() == ("auto", "two-kernel"), sp.get_tree_path()
        st = sp.get_state()
        so.set_trace(True); sp.set_trace(True)
        accepted = 0
        for it in range(2):
            so.set_state(st); sp.set_state(st)
            ro, rp = so.run(1, False, 1), sp.run(1, False, 1)
            to = so.get_trace()
            ctx = f"stationary iteration {it}"
            assert np.array_equal(to, sp.get_trace()), ctx + ": tree-move trace differs"
            np.testing.assert_allclose(ro["bart"]["train"], rp["bart"]["train"], rtol=1e-6, atol=1e-9, err_msg=ctx)
            np.testing.assert_allclose(ro["bart"]["sigma"], rp["bart"]["sigma"], rtol=1e-6, err_msg=ctx)
            assert np.array_equal(ro["bart"]["varcount"], rp["bart"]["varcount"]), ctx
            assert_state_parity(StateView(so.get_state()), StateView(sp.get_state()))
            accepted += int((to[:, 1] == 1).sum())
            st = so.get_state()
        assert accepted < 0.5 * 2 * T, f"not the stationary regime: {accepted} of {2 * T} moves accepted"
    finally:
        sp.free(); so.free()


# ---- probit latents on a long stream ----------------------------------------------------------------------------------------------------------------

def test_probit_latents_at_one_million(oracle_lib, hip_lib):
    """k_latents2 at n = 1.1e6 (the generator's stream ring wraps hundreds of times per draw of the latents), the generator state bit for bit.
    (With the Stan block: a probit model of BART alone is refused as improper.)"""
    args = sized_case(1_100_000, seed=8, trees=4, iters=(2, 5), binary=True, joint=True)
    _parity(oracle_lib, hip_lib, args, "fused", stan=True)
