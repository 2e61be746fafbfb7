"""The persistent sweep's exchange at the edges of its fixed-point format (xc_publish, stan4bart_amd/csrc/dev_step_shared.hpp): every pass workgroup adds
its partial (sum, count) of a bin into copy blockIdx % 8 as two 64-bit words, the sum at an absolute resolution of 2^-55, the count in a 21-bit
field.  Two admissions of the host (dev_hip.hip, creation of the device arrays) keep samplers inside that format, and both are tested at their edges:

  * wRangeOk: k_sweep_w publishes weighted sums times the power of two that brings the largest weight into (0.5, 1].  A bin that holds only the
    lightest observations then has partials of about (their number) * min / max weight, each rounded to 2^-55: a relative error of up to
    2^-55 * max / min.  Samplers whose weights span more than 2^30 take the per-tree kernels, which sum in plain double like the oracle.
  * streamCountOk: the streaming pass (k_sweep_stream) gives a pass workgroup up to ceil(ceil(nQuads / 256) / 255) blocks of 1 024 observations, and
    32 of them share a copy: fewer than 2^16 observations per workgroup keeps a copy's count below 2^21, i.e. n <= 255 * 63 * 1 024 = 16 450 560.
    Beyond, "stream" is refused before anything is launched; the stream path is never run past that n.

Same bar as everywhere: tree-move trace, trees and generator state bit-exact, floating-point state to rtol 1e-6 / atol 1e-9.  Oracle halves on one
CPU core: a few seconds for the weight cases, about 10 s for each of the two stream cases."""
import numpy as np
import pytest

from conftest import assert_chain_parity, friedman_case, make_sampler, run_chain

pytestmark = pytest.mark.gpu

W_RANGE = 2.0 ** -30                          # the smallest min / max weight the weighted persistent sweep takes
N_STREAM_MAX = 255 * 63 * 4 * 256             # 16 450 560: the last n of the streaming pass (255 pass workgroups, 63 blocks of 1 024 each)


# ---- observation weights over a wide range: the admission of k_sweep_w ----------------------------------------------------------------------------

@pytest.mark.parametrize("rho,want", [(2.0 ** -20, "persistent"), (W_RANGE, "persistent"), (np.nextafter(W_RANGE, 0.0), "fused"), (1e-15, "fused")],
                         ids=["2^-20", "at-bound", "just-outside", "1e-15"])
def test_weight_range_picks_the_tree_path(oracle_lib, hip_lib, rho, want):
    """n = 3e5 (147 pass workgroups), weights uniform on (0.5, 1) and 200 of them times `rho`: min / max >= 2^-30 stays on k_sweep_w, a wider range
    takes k_step<weighted> (n = 3e5 is a persistent size, so the per-tree choice is the fused launch); both give the oracle's chain."""
    n = 300_000
    w = np.random.default_rng(11).uniform(0.5, 1.0, n)
    w[:200] = rho * w.max()
    args, _ = friedman_case(n=n, T=6, warmup=3, iter=8, ranef=False, weights=w)
    a = run_chain(oracle_lib, "orc_", args, results_type=1)
    b = run_chain(hip_lib, "s4b_", args, results_type=1)
    assert b["tree_path"] == ("auto", want), b["tree_path"]
    assert (b["sweep_stats"][0] > 0) == (want == "persistent"), b["sweep_stats"]
    assert_chain_parity(a, b, stan=False)
    assert (a["trace"][:, 1] == 1).sum() > 0, "no move was accepted: nothing was tested"


# ---- the count field of the streaming sweep --------------------------------------------------------------------------------------------------------

def _stream_case(n, seed):
    """p = 3 uniform covariates, n.cuts = 100, 3 trees, one warm-up and two sampling iterations, BART block only."""
    from stan4bart_amd import make_sampler_args
    g = np.random.default_rng(920000 + seed)
    x = np.empty((n, 3), order="F")
    for j in range(3):
        x[:, j] = g.random(n)
    y = 10.0 * np.sin(np.pi * x[:, 0] * x[:, 1]) + 20.0 * (x[:, 2] - 0.5) ** 2 + g.standard_normal(n)
    return make_sampler_args(y, x, iter=3, warmup=1, bart_args={"n.trees": 3, "n.cuts": 100})


def _run_created(s, args):
    """run_chain's body for a sampler that already exists (results_type 1, with the trace)."""
    out = {}
    s.set_trace(True)
    out["warmup"] = s.run(args.warmup, True, 1)
    traces = [s.get_trace()]
    s.disengage_adaptation()
    out["sample"] = s.run(args.iter - args.warmup, False, 1)
    traces.append(s.get_trace())
    out["trace"] = np.concatenate(traces)
    out["trees"] = s.get_trees()
    out["rng"] = s.get_r_rng_state()
    out["leaf0"] = s.get_leaf_assignment(0)
    out["range"] = s.get_bart_data_range()
    out["tree_path"] = s.get_tree_path()
    return out


def test_stream_is_refused_past_its_count_bound(oracle_lib, hip_lib):
    """n = 16 450 561: the busiest pass workgroup would stream 64 blocks (65 536 observations), 32 of them 2^21 into one copy.  The request for
    "stream" must fall back (to the fused launch: k_step takes this n) before any run; only then the chain runs and meets the oracle."""
    args = _stream_case(N_STREAM_MAX + 1, seed=1)
    s = make_sampler(hip_lib, "s4b_", args)
    try:
        s.set_tree_path("stream")
        assert s.get_tree_path() in (("stream", "fused"), ("stream", "two-kernel")), s.get_tree_path()
        b = _run_created(s, args)
    finally:
        s.free()
    a = run_chain(oracle_lib, "orc_", args, results_type=1)
    assert_chain_parity(a, b, stan=False)
    assert (a["trace"][:, 1] == 1).sum() > 0, "no move was accepted: nothing was tested"


def test_stream_at_its_count_bound(oracle_lib, hip_lib):
    """n = 16 450 560: 63 blocks (64 512 observations) on each of the first pass workgroups, 2 064 384 in a copy of a root-sized bin."""
    args = _stream_case(N_STREAM_MAX, seed=2)
    a = run_chain(oracle_lib, "orc_", args, results_type=1)
    b = run_chain(hip_lib, "s4b_", args, results_type=1, tree_path="stream")
    assert b["tree_path"] == ("stream", "stream"), b["tree_path"]
    assert b["sweep_stats"][0] > 0, b["sweep_stats"]
    assert_chain_parity(a, b, stan=False)
    assert (a["trace"][:, 1] == 1).sum() > 0, "no move was accepted: nothing was tested"
