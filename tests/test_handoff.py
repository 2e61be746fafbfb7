"""CPU twin of tests/test_gpu_handoff.py: the same hand-off cases (tests/handoff_cases.py) through the test entry s4b_test_hand_off over the emulated
device layer and the oracle — the long-double model against the oracle against the emulation —, the audit of the residual against its own trees over
emulated chains, and what geometry and which host route every case is FOR: HANDOFF_EXPECTED is pinned here by hand, handoff_cases computes it from the
constants it reads from dev_hip.hip, so an edited constant (the 64 coefficients of the one-launch form, BLOCK, the 1 024-workgroup cap) fails this module."""
import numpy as np
import pytest

import handoff_cases as H
from conftest import StateView, binary_case, friedman_case, make_sampler

# name -> (workgroups, trips of the grid-stride loop, ragged last trip, rounds of k_scale's fold of the min / max partials, rounds of its loop over the
# T * node_capacity leaf slots, launches of a hand-off that keeps the scale, launches of one that updates it)
HANDOFF_EXPECTED = {
    "n-1": (1, 1, True, 1, 3, 2, 2),
    "n-3": (1, 1, True, 1, 3, 1, 4),
    "n-255": (1, 1, True, 1, 3, 1, 4),
    "n-256": (1, 1, False, 1, 3, 1, 4),
    "n-257": (1, 2, True, 1, 3, 1, 4),
    "n-1024": (1, 4, False, 1, 3, 1, 4),
    "n-1025": (2, 3, True, 1, 3, 1, 4),
    "n-262145": (257, 4, True, 2, 3, 1, 4),
    "n-1049385": (1024, 5, True, 4, 3, 1, 4),
    "ext-first-last": (3, 4, True, 1, 3, 1, 4),
    "ext-last-first": (3, 4, True, 1, 3, 1, 4),
    "ext-lane63-wave3": (3, 4, True, 1, 3, 1, 4),
    "ext-workgroup-256": (257, 4, True, 2, 3, 1, 4),
    "ext-last-workgroup": (257, 4, True, 2, 3, 1, 4),
    "ext-tie": (257, 4, True, 2, 3, 1, 4),
    "K0-q6": (2, 3, True, 1, 3, 1, 4),
    "q0-K3": (2, 3, True, 1, 3, 1, 4),
    "K12-q52": (2, 3, True, 1, 3, 1, 4),
    "K12-q53": (2, 3, True, 1, 3, 4, 4),
    "z-fixed-3": (2, 3, True, 1, 3, 1, 4),
    "z-ragged": (2, 3, True, 1, 3, 1, 4),
    "off-none": (3, 4, True, 1, 3, 1, 4),
    "off-default": (3, 4, True, 1, 3, 1, 4),
    "off-fixef": (3, 4, True, 1, 3, 1, 4),
    "off-ranef": (3, 4, True, 1, 3, 1, 4),
    "off-bart": (3, 4, True, 1, 3, 1, 4),
    "off-parametric": (3, 4, True, 1, 3, 1, 4),
    "range-shrink-grow": (3, 4, True, 1, 3, 1, 4),
    "range-grow-shrink": (3, 4, True, 1, 3, 1, 4),
    "T1": (2, 3, True, 1, 1, 1, 4),
    "T200-nc256": (2, 3, True, 1, 200, 1, 4),
    "T200-nc1000": (2, 3, True, 1, 782, 1, 4),
    "binary-small": (1, 1, True, 1, 3, 2, 2),
    "binary-3-workgroups": (3, 4, True, 1, 3, 2, 2),
}
CASES = sorted(HANDOFF_EXPECTED)


def expected_of(name, limits=None):
    c = H.build_case(name)
    a = c["args"]
    g = H.geometry(len(a.y), a.n_trees, a.node_capacity or 256, lim=limits)
    return (g["grid"], g["trips"], g["ragged"], g["fold_rounds"], g["slot_rounds"],
            H.hand_off_route(c["K"], c["q"], bool(a.is_binary), False, lim=limits), H.hand_off_route(c["K"], c["q"], bool(a.is_binary), True, lim=limits))


def test_the_constants_are_the_ones_the_cases_were_built_for():
    assert H.handoff_limits() == dict(block=256, inline=64, grid_cap=1024)
    assert sorted(H.case_table()) == CASES


@pytest.mark.parametrize("name", CASES)
def test_case_selects_its_geometry_and_routes(name):
    assert expected_of(name) == HANDOFF_EXPECTED[name], name


def test_a_moved_constant_moves_the_expectations(tmp_path):
    """The pinned table notices an edit of either constant that decides a route or the geometry (handoff_limits on an edited copy of dev_hip.hip)."""
    src = open(H.DEV_HIP).read()
    edits = {"inline": ("K_ + q_ <= 64) {", "K_ + q_ <= 32) {", "double par[64];", "double par[32];", "if (threadIdx.x < 64) par[", "if (threadIdx.x < 32) par["),
             "cap": ("std::min<int64_t>(1024, std::max<int64_t>(1, (nQuads + BLOCK - 1) / BLOCK))", "std::min<int64_t>(512, std::max<int64_t>(1, (nQuads + BLOCK - 1) / BLOCK))")}
    for what, pairs in edits.items():
        text = src
        for old, new in zip(pairs[::2], pairs[1::2]):
            assert old in text
            text = text.replace(old, new)
        p = tmp_path / (what + ".hip")
        p.write_text(text)
        lim = H.handoff_limits(str(p))
        moved = [n for n in CASES if expected_of(n, lim) != HANDOFF_EXPECTED[n]]
        assert moved, what
        assert ("K12-q52" in moved) == (what == "inline") and ("n-1049385" in moved) == (what == "cap")
    p = tmp_path / "reshaped.hip"
    p.write_text(src.replace("if (pendOffset_ && pendSigma_ && !update) {", "if (pendOffset_ && pendSigma_) {"))
    with pytest.raises(AssertionError, match="one-launch form"):
        H.handoff_limits(str(p))


@pytest.mark.parametrize("update", [False, True], ids=["keep", "update"])
@pytest.mark.parametrize("name", CASES)
def test_hand_off_under_the_model(oracle_lib, emul_lib, name, update):
    """model against oracle against emulation: both implementations meet the model's bounds from their own states, and agree with each other on the scale."""
    reports = {}
    outs = {}
    for lib, pfx in ((emul_lib, "emu_"), (oracle_lib, "orc_")):
        reports[pfx] = {}
        outs[pfx] = H.run_case(lib, pfx, name, update, reports[pfx])
        H.assert_case_specifics(name, update, outs[pfx])
    for se, so in zip(outs["emu_"]["scales"][1:], outs["orc_"]["scales"][1:]):
        np.testing.assert_allclose(se, so, rtol=1e-9)
    print(f"hand-off {name} ({'update' if update else 'keep'}): ratios to the bounds, emulation {reports['emu_']}, oracle {reports['orc_']}")


@pytest.mark.parametrize("binary", [False, True], ids=["continuous", "binary"])
def test_create_path(emul_lib, binary):
    rep = {}
    H.check_create(emul_lib, "emu_", binary, rep)
    print(f"create ({'binary' if binary else 'continuous'}): {rep}")


@pytest.mark.parametrize("name", ["K12-q53", "z-ragged"])
def test_parametric_mean(oracle_lib, emul_lib, name):
    for lib, pfx in ((emul_lib, "emu_"), (oracle_lib, "orc_")):
        rep = {}
        H.check_parametric_mean_case(lib, pfx, name, rep)
        print(f"get_parametric_mean {name} {pfx}: {rep}")


def test_the_entry_leaves_the_chain_alone_and_is_refused_on_a_stored_sampler(oracle_lib, emul_lib):
    """Stan's position stays (the blob's NUTS fields are compared in every case); here: a chain goes on after a hand-off, and the refusals."""
    from stan4bart_amd.abi import Sampler, StoredSampler
    args, _ = friedman_case(n=80, T=3, warmup=2, iter=4)
    args.keep_trees = True
    for lib, pfx in ((emul_lib, "emu_"), (oracle_lib, "orc_")):
        s = make_sampler(lib, pfx, args)
        try:
            s.run(2, True)
            K, q = 2, int(sum(int(a) * int(b) for a, b in zip(args.p, args.l)))
            s.test_hand_off(np.zeros(K), np.zeros(q), 0.9, True)
            assert StateView(s.get_state()).get("scale")[3] == pytest.approx(0.9, rel=1e-15)
            s.disengage_adaptation()
            s.run(2, False)
            before = s.get_state()
            with pytest.raises(RuntimeError, match="sigma must be positive"):
                s.test_hand_off(np.zeros(K), np.zeros(q), 0.0, False)
            with pytest.raises(RuntimeError, match="non-finite"):
                s.test_hand_off(np.array([np.nan, 0.0]), np.zeros(q), 1.0, False)
            bad_b = np.zeros(q); bad_b[-1] = np.inf
            with pytest.raises(RuntimeError, match="non-finite"):
                s.test_hand_off(np.zeros(K), bad_b, 1.0, False)
            assert s.get_state() == before, "a refused hand-off changed the state"
            stored = StoredSampler(lib, pfx, s.export_bart_state())
            try:
                with pytest.raises(RuntimeError, match="live sampler"):
                    Sampler.test_hand_off(stored, np.zeros(K), np.zeros(q), 1.0, False)
            finally:
                stored.free()
        finally:
            s.free()


def _weighted():
    from large_cases import sized_case
    return sized_case(1500, seed=3, trees=10, iters=(6, 12), weights=True, joint=True)


AUDITED_CHAINS = {
    "friedman": lambda: friedman_case(n=2000, T=20, warmup=12, iter=24)[0],
    "binary": lambda: binary_case(n=600, T=11, warmup=8, iter=16),
    "modeled-k": lambda: friedman_case(n=500, T=11, warmup=8, iter=16, bart_args={"k": ("chi", 1.25, float("inf"))})[0],
    "thinned": lambda: friedman_case(n=500, T=7, warmup=6, iter=12, skip=3)[0],
    "weighted": _weighted,
    "user-offset": lambda: friedman_case(n=500, T=7, warmup=6, iter=12, offset=np.random.default_rng(4).normal(size=500) * 50.0, offset_type="ranef")[0],
}


@pytest.mark.parametrize("name", sorted(AUDITED_CHAINS))
def test_audit_over_emulated_chains(emul_lib, name):
    args = AUDITED_CHAINS[name]()
    rep = {}
    diag, drifts = H.audited_run(emul_lib, "emu_", args, args.warmup, args.iter - args.warmup, rep)
    assert diag["counters"][1] == args.n_trees * args.n_thin * (args.iter + 1)
    print(f"audit {name}: drift after create / warm-up / at the end {['%.3g' % d for d in drifts]}, largest drift / bound {rep['audit']:.3g}")


def test_the_audit_notices_a_fit_or_a_leaf_value_that_left_the_sum(emul_lib):
    """The power of the audit's third invariant, on states edited through set_state: one observation's total fit off by 1e-9 of the response's range;
    one leaf value of one tree changed by 1e-9 without the residual following.  (set_state rebuilds the leaf planes from the trees, so a wrong leaf
    assignment cannot be planted this way: the routing and count invariants are not tried here.)"""
    args, _ = friedman_case(n=300, T=5, warmup=3, iter=6)
    s = make_sampler(emul_lib, "emu_", args)
    try:
        s.run(3, True)
        led = H.Ledger(args.n_trees, False)
        led.run(3, True)
        H.audit_state(s, args.x_bart, args, led)
        good = s.get_state()
        sv = StateView(good)
        f = sv.get("total_fits"); f[17] += 1e-9
        sv.set("total_fits", f)
        s.set_state(sv.bytes())
        with pytest.raises(AssertionError, match="sum of the assigned leaf values"):
            H.audit_state(s, args.x_bart, args, led)
        s.set_state(good)
        H.audit_state(s, args.x_bart, args, led)
        # a leaf value: the trees follow the last O(N) field of the blob, each as {nodes, leaves} + nodes x 2 int32 + leaves x float64
        sv = StateView(good)
        o, cnt, _ = sv.off["total_fits"]
        o += 8 * cnt
        for t, (nodes, mu) in enumerate(sv.trees):
            o += 8 + 8 * len(nodes)
            if t == 2:
                assert np.frombuffer(sv.b, dtype=np.float64, count=len(mu), offset=o).tolist() == mu.tolist()
                sv.b[o:o + 8] = np.float64(mu[0] + 1e-9).tobytes()
                break
            o += 8 * len(mu)
        s.set_state(sv.bytes())
        assert StateView(s.get_state()).trees[2][1][0] == mu[0] + 1e-9
        with pytest.raises(AssertionError, match="sum of the assigned leaf values"):
            H.audit_state(s, args.x_bart, args, led)
        s.set_state(good)
        H.audit_state(s, args.x_bart, args, led)
    finally:
        s.free()
