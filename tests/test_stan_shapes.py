"""CPU twin of tests/test_gpu_stan_shapes.py: the same parametric-model shapes (tests/large_cases.py: identical data), the product's host logic over the
CPU emulation of the device layer against the oracle.  The emulation has loops of its own, so nothing here says anything about the HIP kernels; what is
pinned here is the HOST side that changes with the same shapes: the Gram matrix of hmc_mode 0 in its three forms (dense: M <= 64 and mostly filled; CSR;
hash map: M * M > 2^22, i.e. M > 2048), the taped gradient that a term with p = 3 selects instead of the closed form (plan_closed_form), weights, K = 0.
Also pinned: which kernel branch every named case is FOR (stan_kernel_branch restates the choice from the constants in dev_hip.hip), so that the GPU
module's cases cannot drift away from the branches they were written for without a failure in the CPU suite."""
import numpy as np
import pytest

from conftest import assert_chain_parity, run_chain, teacher_forced
from large_cases import STAN_LARGE_SHAPES, STAN_SMALL_SHAPES, stan_kernel_branch, stan_shape_case, stan_shape_of

FORCED_ITERS = (40, 46)      # windows of 10 / 10 / 10: the metric changes after transitions 19 and 29; sampling after 40


def forced_args(name, hmc_mode):
    kw = dict(STAN_SMALL_SHAPES[name])
    args = stan_shape_case(seed=sorted(STAN_SMALL_SHAPES).index(name), hmc_mode=hmc_mode, iters=FORCED_ITERS, **kw)
    args.adapt_init_buffer = args.adapt_term_buffer = args.adapt_window = 10
    return args


def free_args(name, hmc_mode):
    kw = dict(STAN_SMALL_SHAPES[name]) if name in STAN_SMALL_SHAPES else dict(STAN_LARGE_SHAPES[name])
    return stan_shape_case(seed=100 + sorted(list(STAN_SMALL_SHAPES) + list(STAN_LARGE_SHAPES)).index(name), hmc_mode=hmc_mode, **kw)


# what every case is for: (fused, KMAX, zFixed, nCopy) and what else its comment in large_cases.py claims
EXPECTED = {
    "K5": (True, 8, 1, 4), "K8": (True, 8, 1, 4), "K8-weighted": (True, 8, 1, 4), "K9": (True, 16, 1, 4), "K16": (True, 16, 1, 4), "K16-weighted": (True, 16, 1, 4),
    "K12-q52": (True, 16, 1, 4), "K12-q53-weighted": (True, 16, 1, 4), "K17": (False, 16, 1, 4), "K20-weighted": (False, 16, 1, 4), "K23": (False, 16, 1, 4),
    "nz4-K8": (True, 8, 4, 4), "nz5-K2": (True, 2, -1, 4), "nz7-K9": (True, 16, -1, 4), "ragged-K5": (True, 8, -1, 4), "K0-sloped": (True, 2, 2, 4),
    "q512-n250": (True, 2, 3, 4), "q513-K5": (True, 8, 1, 1), "q2100-n700k": (True, 4, 1, 1), "q4096-K9": (True, 16, 1, 1), "q4097": (False, 2, 1, 1),
}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_case_selects_the_branch_it_is_named_for(name):
    kw = dict(STAN_SMALL_SHAPES[name]) if name in STAN_SMALL_SHAPES else dict(STAN_LARGE_SHAPES[name])
    if kw["n"] > 10000:
        kw["n"] = 4200          # (the branch does not depend on n; every level stays occupied)
    args = stan_shape_case(seed=0, hmc_mode=0, **kw)
    K, q, nz = stan_shape_of(args)
    assert K == kw["K"] and q == sum(l * (1 + s) for l, s in kw["terms"])
    br = stan_kernel_branch(K, q, nz)
    assert (br["fused"], br["kmax"], br["zfixed"], br["ncopy"]) == EXPECTED[name], br
    if name == "K12-q52":
        assert K + q == 64 and br["par_inline"]
    if name == "K12-q53-weighted":
        assert K + q == 65 and not br["par_inline"]
    if name in ("K17", "K20-weighted", "K23"):
        assert (br["xt_e_launches"], br["xt_e_last"]) == {"K17": (4, 2), "K20-weighted": (5, 1), "K23": (5, 4)}[name], br
    if name == "ragged-K5":
        assert nz == (3, 4), nz             # a varying number of stored entries per row
    if name in ("nz5-K2", "nz7-K9"):
        assert nz == int(name[2]) and max(args.p) == 3          # (p = 3: the taped gradient)
    if name in ("q2100-n700k", "q4096-K9"):
        assert br["lds"] > 48 * 1024, br    # the launch needs the opt-in for more than 48 KiB of dynamic LDS
    if name in ("q512-n250", "q513-K5"):
        assert br["lds"] <= 48 * 1024, br


@pytest.mark.parametrize("hmc_mode", [0, 1])
@pytest.mark.parametrize("name", sorted(STAN_SMALL_SHAPES))
def test_forced_small_shapes(oracle_lib, emul_lib, name, hmc_mode):
    """46 iterations from the oracle's state, through two metric-window ends; deep trajectories must have occurred (hundreds of leapfrogs in one
    iteration: in hmc_mode 1 each is one DIRECT evaluation of the O(N) sums)."""
    rows, ends = teacher_forced(oracle_lib, emul_lib, "emu_", forced_args(name, hmc_mode))
    assert len(ends) >= 2, ends
    assert rows[3].max() >= 6, rows[3]


@pytest.mark.parametrize("hmc_mode", [0, 1])
@pytest.mark.parametrize("name", sorted(STAN_SMALL_SHAPES) + ["q513-K5", "q2100-n700k"])
def test_free_running_shapes(oracle_lib, emul_lib, name, hmc_mode):
    """A short free-running chain (comparable for ~9 iterations); q = 513: the CSR Gram; q = 2100: the hash-map Gram (here at n = 4200)."""
    args = free_args(name, hmc_mode)
    if name == "q2100-n700k":
        kw = dict(STAN_LARGE_SHAPES[name], n=4200)
        args = stan_shape_case(seed=99, hmc_mode=hmc_mode, **kw)
    assert_chain_parity(run_chain(oracle_lib, "orc_", args), run_chain(emul_lib, "emu_", args))
