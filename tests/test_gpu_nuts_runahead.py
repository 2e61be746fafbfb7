"""NUTS run-ahead helpers on the HIP library (stan4bart_amd/csrc/stan_host.hpp, Nuts::RunAhead): a helper thread integrates the backward
direction of a transition on the host while the sampler's thread builds the tree; it never reaches the device layer.  The chain with a helper is
the chain without one bit for bit: Stan rows, sigma, fits, tree-move trace, both generator states and the whole sampler state.  (The cases over the
emulated device layer — both helper counts, the scalar and vector loops, depth limit, divergences, threads, the cap — are in test_nuts_runahead.py.)"""
import os

import numpy as np
import pytest

from conftest import friedman_case, make_sampler

pytestmark = pytest.mark.gpu


def _room_for_a_helper():
    """A sampler whose thread may use one core only (a process bound to a single core) runs without a helper, whatever is asked for: the helper
    would take turns with it on that core.  True if the CPUs this process may use span more than one core."""
    if not hasattr(os, "sched_getaffinity"):
        return True
    cores = set()
    for c in os.sched_getaffinity(0):
        try:
            cores.add(open(f"/sys/devices/system/cpu/cpu{c}/topology/thread_siblings_list").read().strip())
        except OSError:
            cores.add(str(c))
    return len(cores) > 1


ROOM = _room_for_a_helper()

def _chain(hip_lib, args, helpers, warm, iters, wait=False):
    s = make_sampler(hip_lib, "s4b_", args)
    try:
        s.set_nuts_helpers(helpers, wait)
        s.set_trace(True)
        w = s.run(warm, True)
        s.disengage_adaptation()
        r = s.run(iters, False)
        return dict(stan=np.concatenate([w["stan"], r["stan"]], axis=1), sigma=np.concatenate([w["bart"]["sigma"], r["bart"]["sigma"]]),
                    train=np.concatenate([w["bart"]["train"], r["bart"]["train"]], axis=1), trace=s.get_trace(), state=s.get_state(),
                    nuts=s.get_nuts_stats(), grads=int(s.get_counters()[0]), runahead=s.get_nuts_runahead())
    finally:
        s.free()


def _same_with_and_without(hip_lib, args, warm, iters):
    """helpers 0 against 1: as a sampler runs it (a state the helper has not finished in time is computed by the sampler's thread: how many are
    taken depends on the machine's timing), and with the sampler's thread waiting for every backward state (all of them come from the helper)."""
    a = _chain(hip_lib, args, 0, warm, iters)
    assert a["runahead"]["taken"] == 0 and a["runahead"]["transitions_without_helper"] == a["nuts"]["transitions"], a["runahead"]
    for wait in (False, True):
        b = _chain(hip_lib, args, 1, warm, iters, wait)
        for k in ("stan", "sigma", "train", "trace"):
            assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (k, wait)
        assert a["state"] == b["state"], "the sampler states differ"
        assert a["nuts"] == b["nuts"] and a["grads"] == b["grads"]
        if ROOM:
            assert b["runahead"]["transitions_without_helper"] == 0 and (b["runahead"]["taken"] > 0 or not wait), b["runahead"]
        else:
            assert b["runahead"]["taken"] == 0 and b["runahead"]["transitions_without_helper"] == b["nuts"]["transitions"], b["runahead"]
    assert (a["trace"][:, 1] == 1).sum() > 0, "no tree move was accepted"
    return a


def test_same_chain_with_and_without_a_helper(hip_lib):
    """n = 2000, 5 trees, 40 warm-up + 40 sampling iterations, (1 + X4 | g.1) + (1 | g.2)."""
    args, _ = friedman_case(n=2000, slopes=True, T=5, warmup=40, iter=80)
    a = _same_with_and_without(hip_lib, args, 40, 40)
    assert a["stan"][4].max() >= 15, "the case is meant to build trees of several doublings"


def test_same_chain_on_two_workgroups(hip_lib):
    """n = 4097: the Stan block's O(N) sums and the sweep run on two workgroups."""
    args, _ = friedman_case(n=4097, slopes=True, T=5, warmup=10, iter=20)
    _same_with_and_without(hip_lib, args, 10, 10)
