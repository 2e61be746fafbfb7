"""Sweep groups on the GPU (k_sbatch*, dev_sweep.inc; HipSweepGroup, dev_hip.hip): samplers of one process driven from their own threads,
their solo sweeps (n <= 4 096) launched together, one workgroup per member.  Every draw must be the one the ungrouped sampler makes."""
import numpy as np
import pytest

from batch_cases import _assert_same, _run
from conftest import assert_chain_parity, friedman_case, run_chain

pytestmark = pytest.mark.gpu


def _ihdp(**kw):
    from stan4bart_amd.cases import ihdp_case
    a = ihdp_case(**kw)
    a.keep_trees = True
    return a


CASES = {
    "ihdp4": lambda: [(_ihdp(T=75), 100 + c) for c in range(4)],
    "ihdp8": lambda: [(_ihdp(T=75), 200 + c) for c in range(8)],
    "gauss100": lambda: [(friedman_case(n=100, T=20)[0], 300 + c) for c in range(4)],
    "gauss4096": lambda: [(friedman_case(n=4096, T=20, warmup=4, iter=8)[0], 400 + c) for c in range(4)],
    "split_probs": lambda: [(friedman_case(n=600, T=15, bart_args={"split.probs": {0: 4.0, 3: 0.25, 7: 2.0}})[0], 500 + c) for c in range(3)],
    "weights": lambda: [(friedman_case(n=700, T=15, weights=np.random.default_rng(7).uniform(0.2, 3.0, size=700))[0], 600 + c) for c in range(3)],
    "k_chi": lambda: [(friedman_case(n=300, T=12, bart_args={"k": "chi(1.25, Inf)"})[0], 700 + c) for c in range(3)],
    "skip": lambda: [(friedman_case(n=300, T=12, skip=(2, 1))[0], 800 + c) for c in range(3)],
    "mixed_sizes": lambda: [(friedman_case(n=300, T=12)[0], 900), (_ihdp(T=30), 901)],
}


@pytest.mark.parametrize("name", list(CASES))
def test_batched_chains_equal_unbatched(hip_lib, name):
    cases = CASES[name]()
    ref, _ = _run(hip_lib, cases, False)
    got, st = _run(hip_lib, cases, True)
    for a, b in zip(ref, got):
        _assert_same(a, b)
    per = [b["sweeps"] - b["sweeps0"] for b in got]      # the sweeps inside run()
    assert st["batched_sweeps"] == sum(per) and st["unbatched_sweeps"] == 0, (st, per)
    assert st["timeouts"] == 0, st
    # one launch per sweep while every member is inside run(); a member that enters run() late, or is between its warmup and its sampling
    # run, is not waited for, so a few sweeps at those edges go out in launches of their own
    assert max(per) <= st["launches"] < sum(per), (st, per)


def test_one_batched_chain_matches_the_oracle(oracle_lib, hip_lib):
    args = friedman_case(n=300, T=12)[0]
    a = run_chain(oracle_lib, "orc_", args)
    got, st = _run(hip_lib, [(args, 12345)], True)
    b = got[0]
    assert_chain_parity(a, b)
    assert st["batched_sweeps"] == b["sweeps"] - b["sweeps0"] == st["launches"] and st["unbatched_sweeps"] == 0, st


def test_large_n_runs_unbatched(hip_lib):
    """n > 4 096: the multi-workgroup persistent sweep as before; the group counts every sweep as unbatched"""
    cases = [(friedman_case(n=6000, T=12, warmup=3, iter=6)[0], 40 + c) for c in range(2)]
    ref, _ = _run(hip_lib, cases, False)
    got, st = _run(hip_lib, cases, True)
    for a, b in zip(ref, got):
        _assert_same(a, b)
    assert st == dict(launches=0, batched_sweeps=0, unbatched_sweeps=12, timeouts=0), st


def test_stan4bart_batch_chains(hip_lib):
    from stan4bart_amd import stan4bart
    from stan4bart_amd.abi import Sampler
    d = friedman_case(n=200, T=10)[1]
    x = d["x"]
    xb = x[:, [0, 1, 2, 4, 5, 6, 7, 8, 9]]

    def fit(batch):
        return stan4bart(d["y"], xb, X=np.column_stack([x[:, 3], d["z"]]), chains=4, cores=4, seed=3, iter=12, warmup=5,
                         batch_chains=batch, bart_args={"n.trees": 10}, make_sampler=lambda a, st: Sampler(hip_lib, "s4b_", a, st))
    a, b = fit(False), fit(True)
    for name in ("stan", "bart_train", "bart_varcount"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert b.batch_stats["batched_sweeps"] == 4 * 12 and b.batch_stats["unbatched_sweeps"] == 0, b.batch_stats
