"""CPU twin of tests/test_gpu_batch_mixed.py: the cases of tests/batch_cases.py (members of different variants, sizes, schedules, a deep prior,
members that are not eligible) on the emulated device layer, whose sweeps go through the product's rendezvous behind a HostSweepGroup; and the
assertions that keep the case builders honest: the variant of every member under the rule restated from dev_hip.hip."""
import os

import pytest

from batch_cases import (ROOT, BUILDERS, EXPECTED, VARIANT_NAMES, batch_limits, build_case, emulation_eligible, expected_sweeps, phase_variants,
                         run_case, sweep_counts, variant_of)


def test_limits_and_the_sizes_they_give():
    L = batch_limits()
    assert L["pt"] == 64 * L["pw"] and L["last_few"] < L["last_solo"]
    assert L["last_few"] % 4 == 0 and L["last_solo"] % 4 == 0      # (the next n is the first with one more quad)
    assert (L["last_few"] + 3) // 4 == (L["pf"] - 1) * L["pt"] and (L["last_few"] + 4) // 4 == (L["pf"] - 1) * L["pt"] + 1
    assert (L["last_solo"] + 3) // 4 == L["pf"] * L["pt"] and (L["last_solo"] + 4) // 4 == L["pf"] * L["pt"] + 1
    assert len(VARIANT_NAMES) == 5
    # what emulation_eligible restates
    core = open(os.path.join(ROOT, "stan4bart_amd", "csrc", "sampler_core.hpp")).read()
    assert "return n_ <= 4096 && (path[0] == 0 || path[0] == 4); }" in core


@pytest.mark.parametrize("name", list(BUILDERS))
def test_every_member_has_the_variant_the_case_is_for(name):
    L = batch_limits()
    members = build_case(name)
    assert len(members) == len(EXPECTED[name])
    for k, (m, (warm, sample)) in enumerate(zip(members, phase_variants(name))):
        assert variant_of(m.args, "auto", L) == warm, (name, k)
        assert variant_of(m.args, m.switch_to or "auto", L) == sample, (name, k)
        assert len(m.args.y) <= L["last_solo"] + 1 and 5 <= m.args.n_trees <= 12 and 6 <= m.args.iter <= 14, (name, k)


def test_what_the_cases_are_for():
    L = batch_limits()
    n = {name: [len(m.args.y) for m in build_case(name)] for name in BUILDERS}
    ev = {name: [w for w, _ in phase_variants(name)] for name in BUILDERS}
    # one launch with all five kernels, k_sbatch_sp among them at the first n it exists for; the same members joined against the sort's order
    assert ev["five-variants"] == [0, 1, 2, 3, 4] and ev["variant-order"] == [4, 3, 2, 1, 0]
    assert n["five-variants"][:3] == [L["last_few"] + 1, L["last_few"], L["last_few"] + 1]
    assert n["variant-order"] == n["five-variants"][::-1]
    assert len({(m.args.warmup, m.args.iter, m.args.n_thin) for m in build_case("five-variants")}) == 1      # equal schedules
    assert sorted(m.args.n_trees for m in build_case("five-variants")) == [5, 6, 7, 8, 9]
    assert n["size-edges"] == [L["last_few"], L["last_few"] + 1, L["last_solo"], L["last_solo"] + 1]
    # schedules: a binary member, a thinned one, a modeled k, no random effects; iteration counts that all differ
    s = build_case("schedules")
    assert s[0].args.is_binary and s[1].args.n_thin == 2 and s[2].args.k_hyper is not None and len(s[3].args.p) == 0
    assert len({m.args.iter for m in s}) == 4 and len({m.args.n_trees for m in s}) == 4
    assert len(build_case("twelve-members")) == 12 > L["ring"] and len(set(ev["twelve-members"])) == 3
    assert len(set(ev["hand-over"])) == 3 and build_case("hand-over")[0].args.node_capacity == 1024
    assert build_case("hand-over-bart-only")[0].results_type == 1


def _emulation_eligible(m, phase):
    return emulation_eligible(m.args, (m.switch_to or "auto") if phase == 1 else "auto")


@pytest.mark.parametrize("name", list(BUILDERS))
def test_grouped_members_equal_ungrouped_on_the_emulation(emul_lib, name):
    ref, got, st = run_case(emul_lib, "emu_", name)
    # (the emulation counts no sweeps of its own: the group's counters against the schedules)
    on, off = expected_sweeps(name, _emulation_eligible)
    assert st["batched_sweeps"] == on and st["unbatched_sweeps"] == off, (st, on, off)
    assert st["batched_sweeps"] + st["unbatched_sweeps"] == sum(sum(sweep_counts(m)) for m in build_case(name)), st
    per = [sum(c for ph, c in enumerate(sweep_counts(m)) if _emulation_eligible(m, ph)) for m in build_case(name)]
    assert max(per) <= st["launches"] <= sum(per), (st, per)
    if name == "ineligible-beside-eligible":
        assert got[3]["path_mid"][0] == "auto" and got[3]["path_end"][0] == "fused"
    if name.startswith("hand-over"):
        assert got[0]["trace"][:, 4].max() > 32      # trees beyond the 64 node slots: on the GPU these sweeps are handed over
