"""Sweep groups whose members differ, on the GPU (HipSweepGroup::launch, DevHip::sweep_batched_launch / sweep_persistent_finish, k_sbatch* —
stan4bart_amd/csrc/dev_hip.hip, dev_sweep.inc): the cases of tests/batch_cases.py.  One launch holds up to five kernels, each on the slots of
its run of the sorted jobs; members are handed over to k_step launches on their own streams behind a batched launch; members that are not
eligible run beside members that batch; members leave run() while others wait.  Every member's draws are compared bit for bit with the
same members run ungrouped, and one member of every configuration with the CPU oracle at the project's tolerances.

five-variants is the one case that launches k_sbatch_sp (split.probs at the first n that is not `few`) and five kernels in one launch."""
import pytest

from batch_cases import BUILDERS, EXPECTED, build_case, expected_sweeps, phase_variants, run_case, sweep_counts
from conftest import assert_chain_parity, run_chain

pytestmark = pytest.mark.gpu

_RUNS = {}


def _case(hip_lib, name):
    """ungrouped and grouped runs of a case, made once and shared by the tests that read them"""
    if name not in _RUNS:
        _RUNS[name] = run_case(hip_lib, "s4b_", name)
    return _RUNS[name]


@pytest.mark.parametrize("name", list(BUILDERS))
def test_grouped_members_equal_ungrouped(hip_lib, name):
    ref, got, st = _case(hip_lib, name)
    members, phases = build_case(name), phase_variants(name)
    batched, unbatched, per = 0, 0, []
    for k, (m, r, (warm, sample)) in enumerate(zip(members, got, phases)):
        want = sweep_counts(m)
        counted = (r["sweeps_mid"] - r["sweeps0"], r["sweeps"] - r["sweeps_mid"])      # the persistent sweeps inside the two run() calls
        mine = 0
        for ph, ev in enumerate((warm, sample)):
            # every path that counts its sweeps agrees with the schedule (the per-tree kernels count none)
            persistent = (r["path_mid"] if ph == 0 else r["path_end"])[1] == "persistent"
            assert counted[ph] == (want[ph] if persistent else 0), (name, k, ph, counted, want)
            assert persistent or ev is None, (name, k, ph)
            if ev is not None:
                batched += counted[ph]
                mine += counted[ph]
            else:
                unbatched += want[ph]
        if mine:
            per.append(mine)
    assert (batched, unbatched) == expected_sweeps(name), (name, batched, unbatched)
    assert st["batched_sweeps"] == batched and st["unbatched_sweeps"] == unbatched, (st, batched, unbatched)
    assert st["timeouts"] == 0, st
    assert max(per) <= st["launches"] <= sum(per), (st, per)
    if name == "five-variants":      # equal schedules: launches are shared
        assert st["launches"] < sum(per), (st, per)
    if name.startswith("hand-over"):
        for runs in (ref, got):
            assert runs[0]["hand_overs"] - runs[0]["hand_overs0"] > 0, "no sweep of the deep member was handed over inside run()"
            assert runs[1]["hand_overs"] == 0 and runs[2]["hand_overs"] == 0, [r["hand_overs"] for r in runs]
        assert ref[0]["hand_overs"] == got[0]["hand_overs"]
        assert got[0]["trace"][:, 4].max() > 32
        print(f"{name}: {got[0]['hand_overs']} of the deep member's {got[0]['sweeps']} sweeps (the one at creation included) were handed over")
    if name == "ineligible-beside-eligible":
        assert got[3]["path_mid"] == ("auto", "persistent") and got[3]["path_end"] == ("fused", "fused"), (got[3]["path_mid"], got[3]["path_end"])
        assert got[2]["path_end"][1] in ("fused", "two-kernel")
    if name == "size-edges":
        assert got[3]["path_end"][1] == "persistent"      # (the sweep of several workgroups, counted as unbatched)
    print(f"{name}: variants {EXPECTED[name]}, {st}")


# One member of every configuration, from the GROUPED run, against the oracle: (case, member)
ORACLE_MEMBERS = {
    "plain": ("five-variants", 0), "few": ("five-variants", 1), "sp": ("five-variants", 2), "few_sp": ("five-variants", 3),
    "weighted": ("five-variants", 4), "binary": ("schedules", 0), "thinned": ("schedules", 1), "k-chi": ("schedules", 2),
    "deep": ("hand-over-bart-only", 0),
}


@pytest.mark.parametrize("which", list(ORACLE_MEMBERS))
def test_a_grouped_member_matches_the_oracle(oracle_lib, hip_lib, which):
    name, k = ORACLE_MEMBERS[which]
    m = build_case(name)[k]
    b = _case(hip_lib, name)[1][k]
    a = run_chain(oracle_lib, "orc_", m.args, seed=m.seed, results_type=m.results_type)
    if which == "deep":
        assert a["trace"][:, 4].max() > 32 and b["hand_overs"] > 0
        assert_chain_parity(a, b, stan=False)      # (the BART block alone, as the member's ungrouped test compares it)
    else:
        assert_chain_parity(a, b)
