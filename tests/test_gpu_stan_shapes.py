"""The O(N) kernels of the Stan block (ss = e'We, X'We, Z'We: once per Gibbs iteration and, in hmc_mode 1, once per leapfrog) against the oracle at the
parametric-model shapes that select them.  Which kernel runs, which template instantiation and which branch inside it is decided by K (columns of X),
q (columns of Z) and the non-zeros per row of Z alone (stan4bart_amd/csrc/dev_hip.hip):
  * fused (k_stan_fused, fixed-point sums) while K <= 16 and q <= S_QMAX = 4096; instantiation KMAX = 2 / 4 / 8 / 16 by K; otherwise the plain-double
    pipeline k_stan_inputs + k_xt_e (columns 3.., four per launch) + k_zt_chunks + k_stan_finalize is the primary path;
  * rows of Z that all store the same number z <= S_ZMAX = 4 of entries are kept in registers (zFixed = z), anything else walks the CSR arrays;
  * q <= 512: one LDS histogram of Z'e per wave, above: one shared by the four waves; above q = 2048 the launch asks for more than 48 KiB of LDS;
  * K + q <= S_PAR_INLINE = 64: beta, b travel in the kernel arguments of a leapfrog, above: they are read from device memory.
Every other module of the suite builds K <= 3 with at most 3 stored entries per row, i.e. <2> / <4>, zFixed 0 .. 3, and never launches k_xt_e.
The cases are the ones of tests/large_cases.py (the CPU twin tests/test_stan_shapes.py runs the same data over the emulation and pins which branch every
case is for).  Every test here asserts from get_fused_stats that the path it was written for was taken; the branch inside the kernel is not reported by
the C-ABI, it is DERIVED here from (K, q, row lengths) by stan_kernel_branch, which reads the constants from dev_hip.hip: if a threshold moves, the
expectation below fails instead of the case quietly testing another branch.
Same bar as everywhere: tree-move trace, generator state, treedepth / n_leapfrog / divergent bit-exact, floating-point state to rtol 1e-6 / atol 1e-9.
Two forms: a short free-running chain (comparable for ~9 iterations, early iterations take a few leapfrogs each) and, for the small-q shapes, 46
teacher-forced iterations with adaptation windows of 10 in which trajectories of treedepth >= 6 must occur (in hmc_mode 1: hundreds of DIRECT
evaluations in one iteration).  The oracle differentiates in forward mode, O(D^2) per evaluation with D ~ K + q: at q = 4096 its evaluations take a good
part of a second each, which is why the large-q chains are 4 - 6 iterations and the oracle's chain (it has no hmc_mode) is computed once for both modes."""
import conftest
import numpy as np
import pytest

from conftest import assert_chain_parity, run_chain, teacher_forced
from large_cases import STAN_LARGE_SHAPES, STAN_SMALL_SHAPES, stan_kernel_branch, stan_shape_of
from test_stan_shapes import EXPECTED, forced_args, free_args

pytestmark = pytest.mark.gpu

_oracle_chains = {}


def _oracle_chain(oracle_lib, name, args):
    if name not in _oracle_chains:
        _oracle_chains[name] = run_chain(oracle_lib, "orc_", args)
    return _oracle_chains[name]


def _assert_path(name, args, fused_stats, min_evals):
    """The path from what the C-ABI reports, the branch from the shape."""
    K, q, nz = stan_shape_of(args)
    br = stan_kernel_branch(K, q, nz)
    assert (br["fused"], br["kmax"], br["zfixed"], br["ncopy"]) == EXPECTED[name], (name, br)
    evals, fallbacks = fused_stats
    print(f"{name} hmc_mode {args.hmc_mode}: K {K} q {q} nz {nz} branch {br} fused evaluations {evals} fallbacks {fallbacks}")
    if br["fused"]:
        assert evals >= min_evals, (evals, min_evals)
        assert fallbacks < evals, (evals, fallbacks)
    else:
        assert evals == 0, fused_stats          # K > 16 or q > S_QMAX: every sum came from the plain-double pipeline
    return br


@pytest.mark.parametrize("hmc_mode", [0, 1])
@pytest.mark.parametrize("name", sorted(STAN_SMALL_SHAPES) + sorted(STAN_LARGE_SHAPES))
def test_free_running(oracle_lib, hip_lib, name, hmc_mode):
    args = free_args(name, hmc_mode)
    a = _oracle_chain(oracle_lib, name, args)
    b = run_chain(hip_lib, "s4b_", args)
    assert_chain_parity(a, b)
    leapfrogs = int(a["warmup"]["stan"][4].sum() + a["sample"]["stan"][4].sum())
    # hmc_mode 0: one evaluation per Gibbs iteration (the sufficient statistics); hmc_mode 1: one more per leapfrog (and the ones of init_stepsize)
    _assert_path(name, args, b["fused_stats"], args.iter + (leapfrogs if hmc_mode == 1 else 0))
    if name == "q2100-n700k":
        assert len(args.y) > 2048 * 256         # more observations than the largest grid has threads: the grid-stride loop goes round
    if name == "q512-n250":
        assert len(args.y) < 256


@pytest.mark.parametrize("hmc_mode", [0, 1])
@pytest.mark.parametrize("name", sorted(STAN_SMALL_SHAPES))
def test_forced_through_deep_trajectories(oracle_lib, hip_lib, monkeypatch, name, hmc_mode):
    args = forced_args(name, hmc_mode)
    stats = {}
    make = conftest.make_sampler

    def make_and_watch(lib, prefix, a, seed=12345):          # (teacher_forced frees its samplers: read the diagnostics of the HIP one just before)
        s = make(lib, prefix, a, seed)
        if prefix == "s4b_":
            free = s.free

            def free_after_reading():
                stats["fused"] = s.get_fused_stats()
                free()
            s.free = free_after_reading
        return s
    monkeypatch.setattr(conftest, "make_sampler", make_and_watch)
    rows, ends = teacher_forced(oracle_lib, hip_lib, "s4b_", args)
    assert len(ends) >= 2, ends
    assert rows[3].max() >= 6, rows[3]          # deep trajectories really occurred
    print(f"{name}: max treedepth {int(rows[3].max())}, leapfrogs {int(rows[4].sum())}")
    _assert_path(name, args, stats["fused"], args.iter + (int(rows[4].sum()) if hmc_mode == 1 else 0))
