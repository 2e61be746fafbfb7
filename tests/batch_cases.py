"""Sweep groups whose members DIFFER (HipSweepGroup::launch, k_sbatch* — stan4bart_amd/csrc/dev_hip.hip, dev_sweep.inc; the rendezvous of
stan4bart_amd/csrc/sweep_group.hpp): the driver, the equality, the rule that gives a member its batched kernel and the case builders shared by
tests/test_gpu_batch.py, tests/test_gpu_batch_mixed.py (libs4b.so on the GPU) and the CPU twin tests/test_batch_mixed.py (the emulated device layer
behind a HostSweepGroup).

A group promises that every draw is the one the chain makes alone, so the reference of every case is the same members run ungrouped, and the
comparison has no tolerance: bits.

What picks a member's kernel (restated by variant_of, its statements asserted to still be in the source by batch_limits):
    nQuads = ceil(n / 4);  solo = nQuads <= SW_PT * SW_PF (one workgroup);  few = nQuads <= (SW_PF - 1) * SW_PT (no pass thread owns SW_PF quads)
    eligible = the persistent path, one workgroup, not the streaming pass; weights together with split.probs never take the persistent path
    variant  = 4 weighted, else split.probs ? (few ? 3 : 2) : (few ? 1 : 0)          kern[5] = k_sbatch, _few, _sp, _few_sp, _w
A launch sorts its jobs by variant and launches one kernel per run of equal variants, each on the slots of its run: cases with more than one variant
are the only ones in which a kernel's slot pointer is not the start of the buffer.

A rendezvous bug must end as a failed assertion, not as a hung test: every member is created and joined before any member calls run() (a barrier),
threads are daemon threads joined with a bound, groups get a timeout of 20 s and every case asserts that no wait ran into it."""
import copy
import os
import re
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_HIP = os.path.join(ROOT, "stan4bart_amd", "csrc", "dev_hip.hip")
SWEEP_API = os.path.join(ROOT, "stan4bart_amd", "csrc", "dev_sweep_api.hpp")
GROUP_TIMEOUT_S = 20.0
JOIN_BOUND_S = 120.0
VARIANT_NAMES = ("plain", "few", "sp", "few_sp", "weighted")


class Member:
    """One member of a case: sampler arguments, the seed of its generator, and what its thread does beyond two run() calls.
    results_type: as run() takes it (0 joint, 1 the BART block alone); switch_to: the tree path set between the warm-up and the sampling run."""

    def __init__(self, args, seed, results_type=0, switch_to=None):
        self.args, self.seed, self.results_type, self.switch_to = args, int(seed), int(results_type), switch_to


def _member(m):
    return m if isinstance(m, Member) else Member(*m)


# ---- the driver --------------------------------------------------------------------------------------------------------------------------------
def _chain(lib, prefix, member, group, out, k, barrier):
    from stan4bart_amd import RRng
    from stan4bart_amd.abi import Sampler
    r, s, joined = {}, None, False
    try:
        args = copy.copy(member.args)
        rng = RRng(member.seed)
        args.seed = int(rng.sample_int(2147483647, 1)[0])
        s = Sampler(lib, prefix, args, rng.state)
        r["sweeps0"], r["hand_overs0"] = (int(v) for v in s.get_sweep_stats())      # (sweeps made at creation, before the sampler joined)
        s.set_trace(True)
        if group is not None:
            group.join(s)
            joined = True
        barrier.wait(JOIN_BOUND_S)                      # every member is created and joined before any member runs
        traces = []
        if args.warmup > 0:
            r["warmup"] = s.run(args.warmup, True, member.results_type)
            traces.append(s.get_trace())
        r["sweeps_mid"] = int(s.get_sweep_stats()[0])
        r["path_mid"] = s.get_tree_path()
        s.disengage_adaptation()
        if member.switch_to is not None:
            s.set_tree_path(member.switch_to)
        r["sample"] = s.run(args.iter - args.warmup, False, member.results_type)
        traces.append(s.get_trace())
        r["trace"] = np.concatenate(traces)
        r["trees"] = s.get_trees()
        if getattr(args, "keep_trees", False):
            r["kept_trees"] = s.get_kept_trees()
        r["rng"] = s.get_r_rng_state()
        r["leaf0"] = s.get_leaf_assignment(0)
        r["range"] = s.get_bart_data_range()
        r["pm"] = s.get_parametric_mean()
        r["sweeps"], r["hand_overs"] = (int(v) for v in s.get_sweep_stats())
        r["path_end"] = s.get_tree_path()
    except Exception as e:      # noqa: BLE001  (surfaced by the caller)
        r["error"] = e
        barrier.abort()         # (a member that fails before the barrier must not leave the others waiting at it)
    finally:
        try:
            if joined:
                group.leave(s)
        finally:
            if s is not None:
                s.free()
    out[k] = r


def _run(lib, cases, grouped, prefix="s4b_", timeout_s=GROUP_TIMEOUT_S):
    """cases: [Member or (args, seed)], each chain in a thread of its own; grouped: all in one sweep group.  Returns (results, group stats)."""
    from stan4bart_amd.abi import SweepGroup
    members = [_member(m) for m in cases]
    g = SweepGroup(lib, prefix, 0, len(members)) if grouped else None
    if g is not None:
        g.set_timeout(timeout_s)
    out = {}
    barrier = threading.Barrier(len(members))
    th = [threading.Thread(target=_chain, args=(lib, prefix, m, g, out, k, barrier), daemon=True) for k, m in enumerate(members)]
    [t.start() for t in th]
    deadline = time.monotonic() + JOIN_BOUND_S
    [t.join(max(0.0, deadline - time.monotonic())) for t in th]
    assert not any(t.is_alive() for t in th), "a chain did not finish"
    for k in range(len(members)):
        assert "error" not in out[k], (k, out[k].get("error"))
    st = None
    if g is not None:
        st = g.stats()
        g.free()
    return [out[k] for k in range(len(members))], st


def _assert_same(a, b):
    """bit-identical: the batched launch runs exactly the member's own sweep"""
    assert np.array_equal(a["trace"], b["trace"])
    assert np.array_equal(a["rng"], b["rng"])
    for k in ("tree", "n", "var", "split", "value"):
        assert np.array_equal(a["trees"][k], b["trees"][k]), k
    assert np.array_equal(a["leaf0"], b["leaf0"])
    for ph in ("warmup", "sample"):
        if ph not in a:
            continue
        x, y = a[ph].get("stan"), b[ph].get("stan")              # (none from a run of the BART block alone)
        assert (x is None and y is None) or np.array_equal(x, y), ph
        for f in ("train", "test", "varcount"):
            x, y = a[ph]["bart"].get(f), b[ph]["bart"].get(f)
            assert (x is None and y is None) or np.array_equal(x, y), (ph, f)
    if "kept_trees" in a:
        for k in a["kept_trees"]:
            assert np.array_equal(a["kept_trees"][k], b["kept_trees"][k]), k


# ---- which batched kernel a member takes -------------------------------------------------------------------------------------------------------
def batch_limits(dev_hip=DEV_HIP, sweep_api=SWEEP_API):
    """SW_PW, SW_PF (read from dev_sweep_api.hpp), the sizes they give, and the ring of slot buffers; the statements variant_of restates are asserted
    to still be in dev_hip.hip, so that a moved threshold fails here instead of quietly moving the cases."""
    api, src = open(sweep_api).read(), open(dev_hip).read()
    lim = dict(pw=int(re.search(r"constexpr int SW_PW = (\d+);", api).group(1)), pf=int(re.search(r"constexpr int SW_PF = (\d+);", api).group(1)))
    assert "constexpr int SW_PT = SW_PW * 64;" in api, "SW_PT is no longer SW_PW waves of 64 pass threads"
    lim["pt"] = lim["pw"] * 64
    for stmt in ("const int64_t nQuads = (n_ + 3) / 4;",
                 "sweepSolo_ = nQuads <= (int64_t)SW_PT * SW_PF;",
                 "sweepFew_ = nQuads <= (int64_t)(SW_PF - 1) * (sweepSolo_ ? 1 : a.gridF - 1) * SW_PT;",
                 "sweepGrid_ = (path_ == PATH_SWEEP && sweepSolo_) ? 1 : a_.gridF;",
                 "bool group_eligible() const { return is_persistent() && sweepGrid_ == 1 && !sweepStream_; }",
                 "int batch_variant() const { return weighted_ ? 4 : (splitProbs_ ? (sweepFew_ ? 3 : 2) : (sweepFew_ ? 1 : 0)); }",
                 "static void (*const kern[5])(const unsigned char*) = {k_sbatch, k_sbatch_few, k_sbatch_sp, k_sbatch_few_sp, k_sbatch_w};",
                 "const bool common = stepOk && !(weighted_ && (splitProbs_ || !weightedSweepBuilt || !wScaleOk || !wRangeOk)) &&",
                 "(const unsigned char*)(dev_[r] + b0 * SW_SLOT_BYTES));"):
        assert stmt in src, stmt
    lim["ring"] = int(re.search(r"static constexpr int RING = (\d+);", src).group(1))
    lim["last_few"] = 4 * (lim["pf"] - 1) * lim["pt"]          # the last n whose sweep no pass thread owns SW_PF quads of
    lim["last_solo"] = 4 * lim["pt"] * lim["pf"]               # the last n of the one-workgroup sweep
    return lim


def variant_of(args, tree_path="auto", lim=None):
    """The batched kernel of a sampler made from `args` while `tree_path` is requested: 0 plain, 1 few, 2 sp, 3 few_sp, 4 weighted; None for a
    sampler that is in the group but not eligible (its sweeps are launched on their own and nobody waits for it)."""
    L = lim or batch_limits()
    if tree_path not in ("auto", "persistent"):
        return None
    weighted, sp = args.weights is not None, args.split_probs is not None
    if weighted and sp:
        return None                                            # (no persistent sweep: the per-tree kernels)
    quads = (len(args.y) + 3) // 4
    if quads > L["pt"] * L["pf"]:
        return None                                            # (the sweep of several workgroups)
    few = quads <= (L["pf"] - 1) * L["pt"]
    return 4 if weighted else ((3 if few else 2) if sp else (1 if few else 0))


def emulation_eligible(args, tree_path="auto"):
    """What the member of a HostSweepGroup goes by (SamplerCore::group_eligible without batched kernels): the size and the requested path alone."""
    return len(args.y) <= 4096 and tree_path in ("auto", "persistent")


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
SPLIT_PROBS = {0: 4.0, 3: 0.25, 7: 2.0}


def _friedman(n, T, warmup=4, iter=8, sp=False, weights=False, **kw):
    from conftest import friedman_case
    if sp:
        kw["bart_args"] = dict(kw.get("bart_args", {}), **{"split.probs": SPLIT_PROBS})
    if weights:
        kw["weights"] = np.random.default_rng(7).uniform(0.2, 3.0, size=n)
    a = friedman_case(n=n, T=T, warmup=warmup, iter=iter, **kw)[0]
    a.keep_trees = True
    return a


def deep_member(seed, results_type=0):
    """The member of test_hand_over_from_the_one_workgroup_sweep (tests/test_gpu_parity.py): trees that outgrow the 64 node slots of the
    wave-register path, so that sweeps are handed over to k_step launches on the member's own stream."""
    from stan4bart_amd import make_sampler_args
    g = np.random.default_rng(3738)
    n = 2317
    xb = np.column_stack([g.normal(size=n), g.random(n), (g.random(n) < 0.3).astype(np.float64)])
    x4 = g.random(n)
    y = 3.0 * np.sin(2.0 * xb[:, 0]) + 2.0 * (xb[:, 2] > 0.5) + 1.5 * x4 + g.normal(size=n)
    args = make_sampler_args(y, xb, X=x4[:, None], groups=[], iter=14, warmup=6,
                             bart_args={"n.trees": 8, "n.cuts": 5, "k": 0.3, "base": 0.99, "power": 0.25})
    args.node_capacity = 1024
    return Member(args, seed, results_type=results_type)


def _five(seed0):
    """plain, few, sp, few_sp, weighted: in the order of the variants"""
    L = batch_limits()
    few, first = L["last_few"], L["last_few"] + 1
    return [Member(_friedman(first, 5), seed0), Member(_friedman(few, 6), seed0 + 1), Member(_friedman(first, 7, sp=True), seed0 + 2),
            Member(_friedman(600, 8, sp=True), seed0 + 3), Member(_friedman(700, 9, weights=True), seed0 + 4)]


def _five_variants():
    return _five(1100)


def _variant_order():
    m = _five(1200)
    return [m[4], m[3], m[2], m[1], m[0]]


def _variant_order_alternating():
    L = batch_limits()
    return [Member(_friedman(L["last_few"] + 1, 5), 1300), Member(_friedman(700, 6, weights=True), 1301),
            Member(_friedman(L["last_solo"], 7), 1302), Member(_friedman(333, 8, weights=True), 1303)]


def _size_edges():
    L = batch_limits()
    return [Member(_friedman(n, 6, warmup=3, iter=6), 1400 + k)
            for k, n in enumerate((L["last_few"], L["last_few"] + 1, L["last_solo"], L["last_solo"] + 1))]


def _ineligible_beside_eligible():
    return [Member(_friedman(300, 6), 1500), Member(_friedman(517, 7), 1501),
            Member(_friedman(400, 6, sp=True, weights=True), 1502),            # weights with split.probs: the per-tree kernels
            Member(_friedman(350, 6), 1503, switch_to="fused")]                # eligible in its warm-up run, not in its sampling run


def _schedules():
    from conftest import binary_case
    b = binary_case(n=300, T=5, warmup=3, iter=6)
    b.keep_trees = True
    return [Member(b, 1600), Member(_friedman(300, 12, warmup=4, iter=9, skip=(2, 1)), 1601),
            Member(_friedman(300, 8, warmup=5, iter=12, bart_args={"k": "chi(1.25, Inf)"}), 1602),
            Member(_friedman(450, 10, warmup=6, iter=14, ranef=False), 1603)]


def _hand_over(results_type=0):
    return [deep_member(1700, results_type), Member(_friedman(batch_limits()["last_few"] + 1, 6, warmup=6, iter=14), 1701),
            Member(_friedman(700, 7, warmup=6, iter=14, weights=True), 1702)]


def _hand_over_bart_only():
    return _hand_over(results_type=1)


def _twelve_members():
    kinds = (dict(), dict(sp=True), dict(weights=True))
    return [Member(_friedman(100, 5, **kinds[k % 3]), 1800 + k) for k in range(12)]


BUILDERS = {
    "five-variants": _five_variants,
    "variant-order": _variant_order,
    "variant-order-alternating": _variant_order_alternating,      # (the second run of variant-order: plain, weighted, plain, weighted)
    "size-edges": _size_edges,
    "ineligible-beside-eligible": _ineligible_beside_eligible,
    "schedules": _schedules,
    "hand-over": _hand_over,
    "hand-over-bart-only": _hand_over_bart_only,                  # (the deep member as its ungrouped test runs it, for the comparison with the oracle)
    "twelve-members": _twelve_members,
}

# The variant of every member of every case (None: in the group, not eligible; a pair: in the warm-up run, in the sampling run).
EXPECTED = {
    "five-variants": [0, 1, 2, 3, 4],
    "variant-order": [4, 3, 2, 1, 0],
    "variant-order-alternating": [0, 4, 0, 4],
    "size-edges": [1, 0, 0, None],
    "ineligible-beside-eligible": [1, 1, None, (1, None)],
    "schedules": [1, 1, 1, 1],
    "hand-over": [1, 0, 4],
    "hand-over-bart-only": [1, 0, 4],
    "twelve-members": [1, 3, 4] * 4,
}

_BUILT = {}


def build_case(name):
    """The members of a case, built once (the threads copy the arguments they run from)."""
    if name not in _BUILT:
        _BUILT[name] = BUILDERS[name]()
    return _BUILT[name]


def phase_variants(name):
    """[(variant in the warm-up run, variant in the sampling run)] of a case's members."""
    return [e if isinstance(e, tuple) else (e, e) for e in EXPECTED[name]]


def sweep_counts(member):
    """(sweeps of the warm-up run, sweeps of the sampling run): one per thinning step of every iteration."""
    a = member.args
    return a.n_thin * a.warmup, a.n_thin * (a.iter - a.warmup)


def expected_sweeps(name, eligible=None):
    """(sweeps of the case's members while eligible, while not), from the schedules alone.  `eligible(member, phase)` replaces EXPECTED's word
    (the emulation's rule differs for weights with split.probs)."""
    on = off = 0
    for m, ev in zip(build_case(name), phase_variants(name)):
        for ph, cnt in enumerate(sweep_counts(m)):
            ok = (ev[ph] is not None) if eligible is None else eligible(m, ph)
            on, off = on + (cnt if ok else 0), off + (0 if ok else cnt)
    return on, off


def run_case(lib, prefix, name):
    """The case ungrouped, then grouped; every member bit-identical.  Returns (ungrouped results, grouped results, the group's counters)."""
    members = build_case(name)
    ref, _ = _run(lib, members, False, prefix)
    got, st = _run(lib, members, True, prefix)
    for k, (a, b) in enumerate(zip(ref, got)):
        try:
            _assert_same(a, b)
        except AssertionError as e:
            raise AssertionError(f"{name}: member {k} (variant {EXPECTED[name][k]}) differs from its ungrouped run: {e}") from e
    assert st["timeouts"] == 0, (name, st)
    return ref, got, st
