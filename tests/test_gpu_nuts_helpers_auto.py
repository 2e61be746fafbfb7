"""The default helper count of the NUTS run-ahead on the HIP library (stan_host.hpp: Nuts::set_helpers_auto): a sampler that nobody gave a count has
one helper, and a second one where the process has the cores for it.  Whatever it comes to, the chain is the helper-less chain bit for bit: Stan
rows, sigma, fits, tree-move trace and the whole sampler state.  (Which count the default comes to on which CPUs: test_nuts_helpers_auto.py.)"""
import os

import numpy as np
import pytest

from conftest import friedman_case, make_sampler

pytestmark = pytest.mark.gpu


def _room_for_a_helper():
    """A sampler whose thread may use one core only runs without a helper, whatever is asked for.  True if the CPUs this process may use span
    more than one core."""
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


def _chain(hip_lib, args, helpers, warm, iters):
    """helpers None: the sampler's default."""
    s = make_sampler(hip_lib, "s4b_", args)
    try:
        if helpers is not None:
            s.set_nuts_helpers(helpers)
        s.set_trace(True)
        w = s.run(warm, True)
        s.disengage_adaptation()
        r = s.run(iters, False)
        return dict(stan=np.concatenate([w["stan"], r["stan"]], axis=1), sigma=np.concatenate([w["bart"]["sigma"], r["bart"]["sigma"]]),
                    train=np.concatenate([w["bart"]["train"], r["bart"]["train"]], axis=1), trace=s.get_trace(), state=s.get_state(),
                    nuts=s.get_nuts_stats(), grads=int(s.get_counters()[0]), runahead=s.get_nuts_runahead())
    finally:
        s.free()


@pytest.mark.parametrize("n", [2000, 6000], ids=["one-workgroup", "two-workgroups"])
def test_same_chain_with_the_default_count(hip_lib, n):
    """5 trees, 20 warm-up + 20 sampling iterations, (1 + X4 | g.1) + (1 | g.2); no helper, the default, both directions."""
    args, _ = friedman_case(n=n, slopes=True, T=5, warmup=20, iter=40)
    ref = _chain(hip_lib, args, 0, 20, 20)
    assert ref["runahead"]["taken"] == 0 and ref["runahead"]["transitions_without_helper"] == ref["nuts"]["transitions"], ref["runahead"]
    for helpers in (None, 2):
        c = _chain(hip_lib, args, helpers, 20, 20)
        for k in ("stan", "sigma", "train", "trace"):
            assert ref[k].shape == c[k].shape and ref[k].tobytes() == c[k].tobytes(), (k, helpers)
        assert ref["state"] == c["state"], f"helpers {helpers}: the sampler states differ"
        assert ref["nuts"] == c["nuts"] and ref["grads"] == c["grads"], helpers
        ra, leapfrogs = c["runahead"], c["nuts"]["sum_n_leapfrog"]
        if ROOM:
            assert ra["transitions_without_helper"] == 0, ra
            assert ra["taken"] + ra["not_ready"] <= leapfrogs, (ra, leapfrogs)
            if helpers == 2:
                assert ra["taken"] + ra["not_ready"] == leapfrogs, (ra, leapfrogs)
        else:
            assert ra["taken"] == 0 and ra["transitions_without_helper"] == c["nuts"]["transitions"], ra
