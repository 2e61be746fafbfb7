"""The Stan -> BART hand-off kernels ALONE on the GPU (k_offset_rescale; k_param_mean + k_set_sigma + k_scale + k_rescale; k_rescale_binary; the create
path; k_param_mean into s.e) through s4b_test_hand_off, against the long-double model of tests/handoff_cases.py at the shapes that select their
branches, with the host route asserted from the launch counter; and the audit of the residual against its own trees after every case and over free
runs on every tree path.  tests/test_handoff.py is the CPU twin (the same cases over the emulation and the oracle; it pins the geometry and the routes)."""
import threading

import numpy as np
import pytest

import handoff_cases as H
from conftest import binary_case, friedman_case

pytestmark = pytest.mark.gpu

CASES = sorted(H.case_table())
RATIOS = {}          # group of cases -> quantity -> largest observed ratio to its derived bound


def _group(name):
    return {"n": "geometry", "ext": "planted extremes", "K0": "K and q", "q0": "K and q", "K12": "K and q", "z": "rows of Z", "off": "offset types",
            "range": "range changes", "T1": "trees", "T200": "trees", "binary": "binary"}[name.split("-")[0]]


def _note(group, rep):
    g = RATIOS.setdefault(group, {})
    for k, v in rep.items():
        g[k] = max(g.get(k, 0.0), v)


@pytest.mark.parametrize("update", [False, True], ids=["keep", "update"])
@pytest.mark.parametrize("name", CASES)
def test_hand_off_under_the_model(hip_lib, name, update):
    rep = {}
    out = H.run_case(hip_lib, "s4b_", name, update, rep)          # (asserts the route: 1, 4 or 2 launches per hand-off)
    H.assert_case_specifics(name, update, out)
    _note(_group(name), rep)
    print(f"hand-off {name} ({'update' if update else 'keep'}): {out['launches']} launches; ratios to the bounds {rep}")


@pytest.mark.parametrize("binary", [False, True], ids=["continuous", "binary"])
def test_create_path(hip_lib, binary):
    rep = {}
    H.check_create(hip_lib, "s4b_", binary, rep)
    _note("create", rep)


@pytest.mark.parametrize("name", ["K12-q53", "z-ragged"])
def test_parametric_mean(hip_lib, name):
    rep = {}
    H.check_parametric_mean_case(hip_lib, "s4b_", name, rep)
    _note("parametric mean", rep)


def test_the_entry_is_refused_on_a_stored_sampler(hip_lib):
    from conftest import make_sampler
    from stan4bart_amd.abi import Sampler, StoredSampler
    args, _ = friedman_case(n=80, T=3, warmup=2, iter=4)
    args.keep_trees = True
    s = make_sampler(hip_lib, "s4b_", args)
    try:
        s.run(2, True)
        s.disengage_adaptation()
        s.run(2, False)
        stored = StoredSampler(hip_lib, "s4b_", s.export_bart_state())
        try:
            with pytest.raises(RuntimeError, match="live sampler"):
                Sampler.test_hand_off(stored, np.zeros(2), np.zeros(int(sum(int(a) * int(b) for a, b in zip(args.p, args.l)))), 1.0, False)
        finally:
            stored.free()
    finally:
        s.free()


# ---- free runs under the audit: (arguments, warm-up, sampling, setup, what the diagnostics must say) ---------------------------------------------------
def _sized(n, **kw):
    from large_cases import sized_case
    return sized_case(n, joint=True, **kw)


def _parallel_latents():
    a = binary_case(n=600, T=11, warmup=8, iter=16)
    a.latents = "parallel"
    return a


def _persistent(d):
    assert d["tree_path"][1] == "persistent" and d["sweep_stats"][0] > 0, d


def _speculating(d):
    _persistent(d)
    launches, decided, published, borne = d["sweep_spec"]
    assert 2 * published > decided > 0, d["sweep_spec"]          # most steps speculate


def _handed_over(d):
    assert d["tree_path"][1] == "persistent" and d["sweep_stats"][1] > 0, d


def _path(name):
    def check(d):
        assert d["tree_path"] == (name, name), d["tree_path"]
        if name in ("fused", "two-kernel"):
            assert d["sweep_stats"] == (1, 0) and d["sweep_spec"][0] == 1, d          # (the sweep inside create, before the path was set, was the only persistent one)
    return check


def _latent(mode):
    def check(d):
        assert d["latent_mode"] == mode, d
    return check


def _busy(d):
    assert d["tree_path"][1] == "persistent" and d["sweep_busy"] > 0, d


FREE_RUNS = {
    "solo-persistent": (lambda: friedman_case(n=2000, T=20, warmup=12, iter=24)[0], None, _persistent),
    "full-grid-1e6-200-trees": (lambda: _sized(1_000_000, trees=200, iters=(3, 5)), None, _speculating),
    "deep-hand-overs": (lambda: _sized(3000, seed=1, trees=20, iters=(4, 8), deep=True), None, _handed_over),
    "k_sweep_w": (lambda: _sized(20000, seed=2, trees=10, iters=(4, 8), weights=True), None, _persistent),
    "k_sweep_sp": (lambda: _sized(20000, seed=3, trees=10, iters=(4, 8), split_probs=True), None, _persistent),
    "stream": (lambda: _sized(20000, seed=4, trees=10, iters=(4, 8)), lambda s: s.set_tree_path("stream"), _path("stream")),
    "fused": (lambda: _sized(20000, seed=5, trees=10, iters=(4, 8)), lambda s: s.set_tree_path("fused"), _path("fused")),
    "two-kernel": (lambda: _sized(20000, seed=6, trees=10, iters=(4, 8)), lambda s: s.set_tree_path("two-kernel"), _path("two-kernel")),
    "binary-exact": (lambda: binary_case(n=600, T=11, warmup=8, iter=16), None, _latent(0)),
    "binary-parallel": (_parallel_latents, None, _latent(1)),
    "modeled-k": (lambda: friedman_case(n=500, T=11, warmup=8, iter=16, bart_args={"k": ("chi", 1.25, float("inf"))})[0], None, _persistent),
    "thinned": (lambda: friedman_case(n=500, T=7, warmup=6, iter=12, skip=3)[0], None, _persistent),
    # (24 000 observations: 6 pass workgroups + the control workgroup, a launch with a roll call — a one-workgroup launch holds none: tests/test_gpu_busy.py)
    "busy-hook": (lambda: friedman_case(n=24_000, T=11, warmup=6, iter=13)[0], lambda s: s.set_test_hook(1, 2), _busy),
}


@pytest.mark.parametrize("name", sorted(FREE_RUNS))
def test_audit_over_free_runs(hip_lib, name):
    build, setup, check = FREE_RUNS[name]
    args = build()
    rep = {}
    diag, drifts = H.audited_run(hip_lib, "s4b_", args, args.warmup, args.iter - args.warmup, rep, setup=setup)
    check(diag)
    assert diag["counters"][1] == args.n_trees * args.n_thin * (args.iter + 1)
    _note("free runs", rep)
    print(f"audit {name}: path {diag['tree_path']}, sweep stats {diag['sweep_stats']}, spec {diag['sweep_spec']}, busy {diag['sweep_busy']}; drift after create / "
          f"warm-up / at the end {['%.3g' % d for d in drifts]}, largest drift / bound {rep['audit']:.3g}")


def test_audit_over_the_members_of_a_sweep_group(hip_lib):
    """Three solo chains in one sweep group, each in a thread of its own: batched sweeps happened, and every member passes the audit at all three points."""
    from stan4bart_amd.abi import SweepGroup
    cases = [friedman_case(n=300 + 100 * k, T=7, warmup=6, iter=12)[0] for k in range(3)]
    g = SweepGroup(hip_lib, "s4b_", 0, len(cases))
    out = {}

    def member(k):
        try:
            rep = {}
            out[k] = H.audited_run(hip_lib, "s4b_", cases[k], 6, 6, rep, setup=g.join, teardown=g.leave, seed=100 + k) + (rep,)
        except BaseException as e:      # noqa: BLE001  (surfaced below)
            out[k] = e
    th = [threading.Thread(target=member, args=(k,)) for k in range(len(cases))]
    [t.start() for t in th]
    [t.join(600) for t in th]
    assert not any(t.is_alive() for t in th), "a member did not finish"
    st = g.stats()
    g.free()
    for k in range(len(cases)):
        if isinstance(out[k], BaseException):
            raise out[k]
        _note("free runs", out[k][2])
    assert st["batched_sweeps"] > 0 and st["launches"] > 0, st
    print(f"audit of a sweep group's members: {st}; drifts {[['%.3g' % d for d in out[k][1]] for k in range(len(cases))]}")


@pytest.fixture(scope="module", autouse=True)
def report_the_largest_ratios():
    """Not a check and not a test: when the module is through, prints (under -s) the largest observed ratio to each derived bound, per group of the
    cases that ran.  The asserted bounds stay the derived ones."""
    yield
    for group in sorted(RATIOS):
        print(f"largest ratios, {group}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(RATIOS[group].items())))
