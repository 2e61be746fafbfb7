"""NUTS run-ahead helpers and the vector forms of the host loops (stan4bart_amd/csrc/stan_host.hpp: Nuts::RunAhead, namespace hostloop) over the
CPU emulation of the device layer.  Neither may change a chain: with 0, 1 or 2 helper threads, with the scalar or the AVX2 loops, the Stan rows,
sigma, the tree-move trace, both generator states and the NUTS totals are the same bit for bit.  Every case runs its reference chain (no helper,
scalar loops) once and compares the other configurations with it."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT, StateView, friedman_case, make_sampler

# (helpers, vector loops, wait) against the reference (0, False).  wait: the sampler's thread waits for every state of a helper's direction, so
# that every one of them comes from the helper whatever the machine's timing; without it a state the helper has not finished in time is computed
# by the sampler's thread, and how many those are depends on the machine.
CONFIGS = [(0, True, False), (1, False, True), (1, True, True), (2, False, True), (2, True, True), (1, True, False), (2, True, False)]


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


def _chain(lib, args, helpers, vector, warm, iters, force_step=None, wait=True):
    """One chain: `warm` warm-up and `iters` sampling iterations.  force_step: the step size is multiplied by it after the warm-up (through the
    state blob).  Returns everything the configurations are compared on, and the run-ahead counters."""
    from stan4bart_amd.abi import set_host_vector
    before = set_host_vector(lib, "emu_", None)
    set_host_vector(lib, "emu_", vector)
    s = make_sampler(lib, "emu_", args)
    try:
        s.set_nuts_helpers(helpers, wait)
        s.set_trace(True)
        w = s.run(warm, True)
        s.disengage_adaptation()
        if force_step is not None:
            sv = StateView(s.get_state())
            nuts = sv.get("nuts"); nuts[0] *= force_step; sv.set("nuts", nuts)
            s.set_state(sv.bytes())
        r = s.run(iters, False)
        sv = StateView(s.get_state())
        return dict(stan=np.concatenate([w["stan"], r["stan"]], axis=1), sigma=np.concatenate([w["bart"]["sigma"], r["bart"]["sigma"]]),
                    trace=s.get_trace(), r_rng=sv.get("r_rng"), ecuyer=sv.get("ecuyer"), nuts=s.get_nuts_stats(), grads=int(s.get_counters()[0]),
                    runahead=s.get_nuts_runahead())
    finally:
        s.free()
        set_host_vector(lib, "emu_", before)


def _same(a, b, ctx):
    for k in ("stan", "sigma", "trace", "r_rng", "ecuyer"):
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), f"{ctx}: {k} differs"
    assert a["nuts"] == b["nuts"] and a["grads"] == b["grads"], f"{ctx}: NUTS totals or gradient count differ"


def _compare_all(lib, args, warm, iters, expect_helper=True, **kw):
    ref = _chain(lib, args, 0, False, warm, iters, **kw)
    assert ref["runahead"]["taken"] == 0 and ref["runahead"]["transitions_without_helper"] == ref["nuts"]["transitions"]
    for helpers, vector, wait in CONFIGS:
        c = _chain(lib, args, helpers, vector, warm, iters, wait=wait, **kw)
        _same(ref, c, f"helpers {helpers}, vector {vector}, wait {wait}")
        ra, leapfrogs = c["runahead"], c["nuts"]["sum_n_leapfrog"]
        if helpers and expect_helper and ROOM:
            assert ra["transitions_without_helper"] == 0 and ra["unconsumed"] >= 0, (helpers, ra)
            if wait:                # the consumed-from-helper counter: every leapfrog of a helper's direction (with two helpers: every leapfrog of a tree)
                assert ra["taken"] > 0 and ra["not_ready"] <= ra["taken"], ra
                assert ra["taken"] == leapfrogs if helpers == 2 else 0 < ra["taken"] < leapfrogs, (ra, leapfrogs)
            else:
                assert ra["taken"] + ra["not_ready"] == leapfrogs if helpers == 2 else ra["taken"] + ra["not_ready"] < leapfrogs, (ra, leapfrogs)
        else:
            assert ra["taken"] == 0 and ra["not_ready"] == 0 and ra["unconsumed"] == 0 and ra["transitions_without_helper"] == c["nuts"]["transitions"], ra
    return ref


def test_deep_trees_same_chain(emul_lib):
    """Friedman n = 200 with (1 + X4 | g.1) + (1 | g.2), 150 warm-up and 100 sampling iterations: trees of depth 7 and more."""
    args, _ = friedman_case(n=200, slopes=True, warmup=150, iter=250)
    ref = _compare_all(emul_lib, args, 150, 100)
    assert ref["stan"][3].max() >= 7, "the case is meant to reach deep trees"


def test_tree_depth_limit_same_chain(emul_lib):
    """max_treedepth = 3: every transition ends at the limit or before it (the helper's array holds 2^3 states)."""
    args, _ = friedman_case(n=200, slopes=True, warmup=40, iter=70)
    args.max_treedepth = 3
    ref = _compare_all(emul_lib, args, 40, 30)
    assert ref["stan"][3].max() == 3 and ref["stan"][4].max() == 7


def test_divergent_transitions_same_chain(emul_lib):
    """a step size forced large after the warm-up: trajectories leave the typical set, energies are not finite, transitions end divergent."""
    args, _ = friedman_case(n=200, slopes=True, warmup=60, iter=90)
    ref = _compare_all(emul_lib, args, 60, 30, force_step=40.0)
    assert ref["nuts"]["divergent"] > 0


def test_model_without_closed_form_runs_without_helper(emul_lib):
    """student-t coefficients are differentiated on the tape: no helper, whatever is asked for, and every transition is counted so."""
    args, _ = friedman_case(n=200, slopes=True, warmup=20, iter=30, stan_args={"prior": dict(dist="student_t", df=5.0)})
    _compare_all(emul_lib, args, 20, 10, expect_helper=False)


def test_hmc_mode_1_runs_without_helper(emul_lib):
    """one device evaluation per leapfrog: a helper thread never calls the device layer, so there is none."""
    args, _ = friedman_case(n=200, slopes=True, warmup=20, iter=30, stan_args={"hmc_mode": 1})
    _compare_all(emul_lib, args, 20, 10, expect_helper=False)


def test_two_samplers_in_two_threads(emul_lib):
    args, _ = friedman_case(n=200, slopes=True, warmup=60, iter=90)
    ref = _chain(emul_lib, args, 0, True, 60, 30)
    out, errs = [None, None], []

    def work(i):
        try:
            out[i] = _chain(emul_lib, args, 1 + i, True, 60, 30, wait=(i == 0))
        except BaseException as e:      # noqa: BLE001 (reported by the test's thread)
            errs.append(e)
    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for i in range(2):
        _same(ref, out[i], f"thread {i}")
    assert out[0]["runahead"]["taken"] > 0 or not ROOM


def test_state_moves_between_samplers_with_and_without_helpers(emul_lib):
    """get_state / set_state carry nothing of a helper: a state taken from a sampler with helpers continues identically in one without, and back."""
    args, _ = friedman_case(n=200, slopes=True, warmup=50, iter=90)
    rows = {}
    for first, second in ((0, 0), (1, 0), (0, 2), (2, 1)):
        a, b = make_sampler(emul_lib, "emu_", args), make_sampler(emul_lib, "emu_", args)
        try:
            a.set_nuts_helpers(first, True); b.set_nuts_helpers(second)
            a.run(50, True)
            b.set_state(a.get_state())
            ra, rb = a.run(20, True), b.run(20, True)
            rows[(first, second)] = (ra["stan"], rb["stan"], a.get_state(), b.get_state())
        finally:
            a.free(); b.free()
    ref = rows[(0, 0)]
    assert ref[0].tobytes() == ref[1].tobytes()
    for key, r in rows.items():
        assert r[0].tobytes() == ref[0].tobytes() and r[1].tobytes() == ref[0].tobytes(), key
        assert r[2] == ref[2] and r[3] == ref[2], key


def test_callback_that_stops_the_run(emul_lib):
    """a callback that raises ends the run between two transitions; the sampler runs on afterwards (same chain as without helpers), and free
    returns: no helper is left running or blocked."""
    class Stop(Exception):
        pass
    finals = {}
    for helpers in (0, 1, 2):
        seen = []

        def cb(tr, te, sp, seen=seen):
            seen.append(sp.copy())
            if len(seen) == 25:
                raise Stop()
        args, _ = friedman_case(n=200, slopes=True, warmup=60, iter=90, callback=cb)
        s = make_sampler(emul_lib, "emu_", args)
        try:
            s.set_nuts_helpers(helpers, True)
            with pytest.raises(Stop):
                s.run(60, True)
            assert len(seen) == 25
            more = s.run(15, True)
            finals[helpers] = (np.array(seen), more["stan"], s.get_state())
            if helpers and ROOM:
                assert s.get_nuts_runahead()["taken"] > 0
        finally:
            s.free()
    for helpers in (1, 2):
        assert finals[helpers][0].tobytes() == finals[0][0].tobytes() and finals[helpers][1].tobytes() == finals[0][1].tobytes()
        assert finals[helpers][2] == finals[0][2]


_CAP_SCRIPT = r"""
import ctypes, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from conftest import friedman_case, make_sampler
lib = ctypes.CDLL(os.path.join(sys.argv[1], "tests", "emul", "_build", "libs4b_emul.so"))
args, _ = friedman_case(n=100, slopes=True, warmup=30, iter=40)
ss = [make_sampler(lib, "emu_", args) for _ in range(9)]
for s in ss: s.set_nuts_helpers(1, True)                        # (waiting: every backward leapfrog is taken from the helper, if there is one)
rows = [s.run(30, True)["stan"].tobytes() for s in ss]          # (every sampler keeps its helper until it is freed)
ra = [s.get_nuts_runahead() for s in ss]
tot = [s.get_nuts_stats()["transitions"] for s in ss]
assert all(r == rows[0] for r in rows), "chains differ"
none = [i for i in range(9) if ra[i]["taken"] == 0]
room = sys.argv[2] == "1"                                        # (a process bound to one core: no sampler has a helper)
assert none == ([8] if room else list(range(9))), (none, ra)
assert ra[8]["transitions_without_helper"] == tot[8] and all(ra[i]["transitions_without_helper"] == (0 if room else tot[i]) for i in range(8)), ra
ss[0].free()                                                     # a freed sampler gives its helper back
more = ss[8].run(5, True)["stan"].tobytes()
assert ss[8].get_nuts_runahead()["taken"] > 0 or not room
assert more == ss[1].run(5, True)["stan"].tobytes()
for s in ss: s.free()
print("cap ok")
"""


def test_nine_samplers_share_eight_helpers(emul_lib):
    """the process-wide cap (a process of its own: the cap counts every sampler alive in a process): the ninth sampler gets no helper, runs inline,
    and its chain is the others' chain."""
    p = subprocess.run([sys.executable, "-c", _CAP_SCRIPT, ROOT, "1" if ROOM else "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0 and "cap ok" in p.stdout, p.stdout


def test_no_data_race_between_sampler_and_helpers(tmp_path):
    """tests/native/nuts_runahead_race.cpp (HostModel + Nuts over a synthetic Gram matrix, no device layer) under ThreadSanitizer, as a child
    process: 200 transitions with 0, 1 and 2 helpers, adapted deep trees and a forced large step with a depth limit of 3; the program also
    compares its chains bit for bit."""
    exe = str(tmp_path / "nuts_runahead_race")
    src = os.path.join(ROOT, "tests", "native", "nuts_runahead_race.cpp")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=thread", "-o", exe, src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([exe, "200"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stdout and r.stdout.strip().endswith("ok"), r.stdout[-4000:]
