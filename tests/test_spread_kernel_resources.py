"""Guard of the register allocation of the spread kernels (stan4bart_amd/csrc/readout_spread.inc), compile only, with the mechanics of
tests/test_projection_kernel_resources.py: the main translation unit is compiled once for the device alone with the product's CXXFLAGS and
`-Rpass-analysis=kernel-resource-usage` is read.

k_spread_reduce keeps the values and weights of 8 rows in flight, their bins and five running statistics per lane; a spill would be paid per row
of every slab.  Its bin tables live in DYNAMIC LDS, (T + 1) KiB sized at launch, so the static LDS of every instance is 0; the instance without
thresholds uses no LDS at all.  k_spread_fold and k_spread_finish keep a handful of sums.  The static LDS and the occupancy are printed, not asserted
(the occupancy that counts at T = 64 is the one the 65 KiB of dynamic LDS leave: two workgroups per CU)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stan4bart_amd", "csrc")

# (mangled prefixes, one per instance: <BINS, SEARCH>)
KERNELS = {"k_spread_reduce<false, false>": "_ZN3s4b15k_spread_reduceILb0ELb0EE", "k_spread_reduce<true, false>": "_ZN3s4b15k_spread_reduceILb1ELb0EE",
           "k_spread_reduce<true, true>": "_ZN3s4b15k_spread_reduceILb1ELb1EE", "k_spread_fold": "_ZN3s4b13k_spread_foldE",
           "k_spread_finish": "_ZN3s4b15k_spread_finishE"}


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
    assert len([b for b in blocks if b.split()[0].startswith("_ZN3s4b15k_spread_reduceILb")]) == 3, "k_spread_reduce has other instances than the three in use"
    found = {}
    for key, prefix in KERNELS.items():
        hit = [b for b in blocks if b.split()[0].startswith(prefix)]
        assert len(hit) == 1, (key, [b.split()[0] for b in blocks])

        def field(name, text=hit[0]):
            return int(re.search(name + r": (\d+)", text).group(1))
        found[key] = dict(vgprs=field("VGPRs"), spill=field("VGPRs Spill"), scratch=field(r"ScratchSize \[bytes/lane\]"),
                          occupancy=field(r"Occupancy \[waves/SIMD\]"), lds=field(r"LDS Size \[bytes/block\]"))
    return found


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_spread_kernels_use_no_private_memory(usage, kernel):
    u = usage[kernel]
    print(f"{kernel}: {u}")
    assert u["spill"] == 0 and u["scratch"] == 0, f"{kernel} uses private memory: {u}"
    assert u["lds"] == 0, f"{kernel} has static LDS (the bin tables are dynamic, sized by T at launch): {u}"


def test_spread_kernels_are_included_after_the_projection_kernels():
    src = open(os.path.join(CSRC, "dev_hip.hip")).read()
    assert '#include "readout_projection.inc"\n#include "readout_spread.inc"\n' in src
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "readout_spread.inc" in mk and mk.count("CXXFLAGS ?=") == 1
    text = open(os.path.join(CSRC, "readout_spread.inc")).read()
    assert not re.search(r"\w*[aA]tomic\w*\s*\(", text), "readout_spread.inc calls an atomic function"
    for k in ("k_spread_reduce", "k_spread_fold", "k_spread_finish"):
        assert f"void {k}(" in text
    # the value kernels of either arm, the chunk rule and the summary over the draws (k_level_rows, k_row_quantiles) are called through the shared helpers
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    for used in ("chunk_plan(", "chunk_grid(", "arm_values_prepare(", "arm_values_launch(", "LevelsSummary sum;", "sum.prepare(", "sum.run("):
        assert used in code, used
    # the summary kernels are used, not copied
    assert "void k_level_rows(" not in text and "void k_row_quantiles(" not in text
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in text and "extern __shared__" in text
