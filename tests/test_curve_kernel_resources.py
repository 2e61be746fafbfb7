"""Guard of the register allocation of the curve kernels (stan4bart_amd/csrc/readout_curves.inc), compile only, with the mechanics of
tests/test_check_kernel_resources.py: the main translation unit is compiled once for the device alone with the product's CXXFLAGS and
`-Rpass-analysis=kernel-resource-usage` is read.

k_curve_values walks four trees at once under the 128 VGPRs that 1024 threads leave; a spill of a vector register to scratch would be paid per tree of
every walk.  The walking kernels of the family spill SCALAR registers into vector lanes (some thirty uniform pointers and counts beside four walks and
the staging exceed the 102 SGPRs of a wave); k_curve_values moves the uniform values its walk does not read into vector registers (cv_vector) and
spills none.  No instance may use private memory, and none may spill a scalar register.  The instances are exactly <staged / global> x <cancelling /
not>: the four that curves_run launches.  k_curve_rows' integer counters are 2 KB of static LDS.  The vector registers and the occupancy are printed,
not asserted (this build: staged cancel 89, global cancel 70, staged 126, global 106, k_curve_rows 31)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stan4bart_amd", "csrc")

# (mangled prefixes, one per instance: <STAGED, CANCEL>)
KERNELS = {f"k_curve_values<{'staged' if st else 'global'}, {'cancel' if ca else 'plain'}>": f"_ZN3s4b14k_curve_valuesILb{st}ELb{ca}EE" for st in (0, 1) for ca in (0, 1)}
KERNELS["k_curve_rows"] = "_ZN3s4b12k_curve_rowsE"


@pytest.fixture(scope="module")
def usage():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not found")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    cxx = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).split()
    cmd = [hipcc, "--offload-arch=gfx950", *cxx, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, "dev_hip.hip"]
    out = subprocess.run(cmd, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:]
    blocks = re.split(r"remark: Function Name: ", out.stdout)[1:]
    assert len([b for b in blocks if b.split()[0].startswith("_ZN3s4b14k_curve_valuesIL")]) == 4, "k_curve_values has other instances than the four in use"
    found = {}
    for key, prefix in KERNELS.items():
        hit = [b for b in blocks if b.split()[0].startswith(prefix)]
        assert len(hit) == 1, (key, [b.split()[0] for b in blocks if "curve" in b.split()[0]])

        def field(name, text=hit[0]):
            return int(re.search(name + r": (\d+)", text).group(1))
        found[key] = dict(vgprs=field("VGPRs"), spill=field("VGPRs Spill"), sgpr_spill=field("SGPRs Spill"), scratch=field(r"ScratchSize \[bytes/lane\]"),
                          occupancy=field(r"Occupancy \[waves/SIMD\]"), lds=field(r"LDS Size \[bytes/block\]"))
    return found


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_curve_kernels_use_no_private_memory(usage, kernel):
    u = usage[kernel]
    print(f"{kernel}: {u}")
    assert u["spill"] == 0 and u["scratch"] == 0, f"{kernel} uses private memory: {u}"
    assert u["sgpr_spill"] == 0, f"{kernel} spills scalar registers into vector lanes: {u}"
    assert u["lds"] == (2 * 4 * 64 * 4 if kernel == "k_curve_rows" else 0), f"{kernel}: static LDS {u}"


def test_curve_kernels_are_included_last_and_share_the_family_routines():
    src = open(os.path.join(CSRC, "dev_hip.hip")).read()
    assert '#include "readout_check.inc"\n#include "readout_curves.inc"\n' in src
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "readout_curves.inc" in mk and mk.count("CXXFLAGS ?=") == 1
    text = open(os.path.join(CSRC, "readout_curves.inc")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert set(re.findall(r"\w*[aA]tomic\w*", code)) == {"atomicAdd"} and code.count("atomicAdd(&cnt[") == 2, "other atomics than the two integer LDS counters"
    assert re.search(r"__shared__ int cnt\[", code)
    for k in ("k_curve_values", "k_curve_rows"):
        assert f"void {k}(" in text
    # the walk, the staging, the summary kernels are used, not copied
    for used in ("walk_trees<STAGED, true, true>(", "walk_trees<STAGED, false, true>(", "stage_draw<true>(", "add_linear(", "readout_phi(", "readout_plan(",
                 "chunk_plan(", "chunk_grid(", "LevelsSummary sum;", "sum.prepare(", "sum.run("):          # (k_level_rows, k_row_quantiles: through LevelsSummary)
        assert used in code, used
    for copied in ("void k_level_rows(", "void k_row_quantiles(", "double walk_trees(", "void stage_draw(", "void qt_sort_rows("):
        assert copied not in text, copied
    # the anchor's value and every grid point's go through one routine: the same bits
    assert code.count("double curve_point(") == 1 and code.count("curve_point<STAGED, CANCEL>(") == 2
