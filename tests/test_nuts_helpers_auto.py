"""The automatic count of NUTS run-ahead helpers (stan4bart_amd/csrc/stan_host.hpp: Nuts::set_helpers_auto, CpuNeighbours::helper_set) over the CPU
emulation of the device layer.  A sampler that nobody gave a helper count (S4B_NUTS_HELPERS unset, s4b_set_nuts_helpers not called) has one helper,
and a second one where the CPUs a helper can be put on span two cores, the process may use three cores for every live sampler that may run ahead and
the budget has room.  Each case runs in a child process bound to chosen CPUs; the chains of all samplers of a case are the same."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

# How many helpers a sampler has shows in its run-ahead counters: none — every transition is counted as without a helper; both directions — every
# leapfrog of every tree was either taken from a helper or found not ready; one — fewer than all of them (the forward leapfrogs belong to nobody).
_POLICY_SCRIPT = r"""
import ctypes, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
cpus = [int(c) for c in sys.argv[2].split(",")]
os.sched_setaffinity(0, cpus)
from conftest import friedman_case, make_sampler
lib = ctypes.CDLL(os.path.join(sys.argv[1], "tests", "emul", "_build", "libs4b_emul.so"))
n_samplers, expect = int(sys.argv[3]), int(sys.argv[4])
args, _ = friedman_case(n=100, slopes=True, warmup=40, iter=50)
ss = [make_sampler(lib, "emu_", args) for _ in range(n_samplers)]        # (all alive before any of them runs)
rows = [s.run(40, True)["stan"].tobytes() for s in ss]
for s in ss:
    ra, tot = s.get_nuts_runahead(), s.get_nuts_stats()
    served = ra["taken"] + ra["not_ready"]
    if ra["transitions_without_helper"] == tot["transitions"]: have = 0
    elif served == tot["sum_n_leapfrog"] and ra["transitions_without_helper"] == 0: have = 2
    else: have = 1
    assert have == expect, (have, expect, ra, tot)
assert all(r == rows[0] for r in rows), "chains differ"
ss[0].set_nuts_helpers(0)                                                # an explicit setting ends the automatic count
more = ss[0].run(5, True)["stan"].tobytes()
assert ss[0].get_nuts_runahead()["transitions_without_helper"] >= 5
if n_samplers > 1:
    assert more == ss[1].run(5, True)["stan"].tobytes(), "chains differ after the explicit setting"
for s in ss: s.free()
print("policy ok")
"""


def _siblings(c):
    """the hardware threads of CPU c's core (the CPU alone where the topology cannot be read)"""
    try:
        txt = open(f"/sys/devices/system/cpu/cpu{c}/topology/thread_siblings_list").read().strip()
    except OSError:
        return frozenset([c])
    return frozenset(_parse(txt))


def _parse(txt):
    out = set()
    for part in txt.split(","):
        lo, _, hi = part.partition("-")
        out.update(range(int(lo), int(hi or lo) + 1))
    return out


def _cache_mates(c):
    """CPUs under the last-level cache of CPU c, or None where the topology cannot be read."""
    try:
        return _parse(open(f"/sys/devices/system/cpu/cpu{c}/cache/index3/shared_cpu_list").read().strip())
    except OSError:
        return None


def _allowed():
    return sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else []


def _one_cpu_per_core(k, one_cache):
    """k CPUs this process may use, of k different cores — under one last-level cache if `one_cache` (that needs the cache topology in sysfs).
    None if there are none."""
    allowed = _allowed()
    for c in allowed:
        mates = _cache_mates(c) if one_cache else set(allowed)
        if mates is None:
            continue
        pick, cores = [], set()
        for m in allowed:
            if m in mates and _siblings(m) not in cores:
                pick.append(m); cores.add(_siblings(m))
        if len(pick) >= k:
            return pick[:k]
        if not one_cache:
            break
    return None


def _policy(cpus, n_samplers, expect):
    env = {k: v for k, v in os.environ.items() if k != "S4B_NUTS_HELPERS"}       # (the default is what is tested)
    p = subprocess.run([sys.executable, "-c", _POLICY_SCRIPT, ROOT, ",".join(str(c) for c in cpus), str(n_samplers), str(expect)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "policy ok" in p.stdout, p.stdout[-4000:]


def _need(k, one_cache):
    cpus = _one_cpu_per_core(k, one_cache)
    if cpus is None:
        pytest.skip(f"needs {k} cores that this process may use" + (" under one last-level cache, with the cache topology readable from sysfs" if one_cache else ""))
    return cpus


def test_one_cpu_no_helper(emul_lib):
    """(needs no cache topology: a thread with no core but its own gets no helper wherever it is)"""
    _policy(_need(1, False), 1, 0)


def test_two_cpus_one_helper(emul_lib):
    """two cores, one CPU of each: one core beside the sampler's, whether or not the two share a cache or the topology can be read"""
    _policy(_need(2, False), 1, 1)


def test_four_neighbouring_cores_two_helpers(emul_lib):
    """the sampler's thread has three neighbour cores wherever it runs, and the process four cores for one sampler"""
    _policy(_need(4, True), 1, 2)


def test_three_samplers_on_four_cores_one_helper_each(emul_lib):
    """four cores are fewer than three for each of three samplers (wherever the four are, and whether or not the cache topology can be read)"""
    cpus = _one_cpu_per_core(4, True) or _need(4, False)      # (under one cache where that can be had: then only the sampler count keeps the second helper away)
    _policy(cpus, 3, 1)


def test_two_cores_with_two_hardware_threads_each_one_helper(emul_lib):
    """a rank bound to two cores of two hardware threads each may use four CPUs, two of them beside the sampler's core — but they are ONE core, and
    two cores are fewer than three: one helper, not two helpers sharing a core.  Needs a machine with such cores under one cache."""
    allowed = set(_allowed())
    for c in sorted(allowed):
        mates = _cache_mates(c)
        if mates is None or len(_siblings(c)) < 2 or not _siblings(c) <= allowed:
            continue
        for m in sorted(allowed):
            if m in mates and _siblings(m) != _siblings(c) and len(_siblings(m)) >= 2 and _siblings(m) <= allowed:
                _policy(sorted(_siblings(c) | _siblings(m)), 1, 1)
                return
    pytest.skip("needs two cores with two hardware threads each under one last-level cache (this machine's cores have one thread, or the topology cannot be read)")
