"""Guard of the register allocation of the projection kernels (stan4bart_amd/csrc/readout_projection.inc), compile only, with the mechanics of
tests/test_groups_kernel_resources.py: the main translation unit is compiled once for the device alone with the product's CXXFLAGS and
`-Rpass-analysis=kernel-resource-usage` is read.

k_proj_reduce<KT> keeps KT + 2 sums of doubles per lane (68 VGPRs of them at KT = 32) and is templated on KT so that they stay in registers: a spill
would be paid per row of every slab.  k_proj_fold keeps one sum.  Neither uses LDS.  k_proj_solve holds the factor in LDS and uses the output matrix as
the substitutions' work space, so that it needs no private memory either.  The occupancy is printed, not asserted."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stan4bart_amd", "csrc")

# (mangled prefixes, one per instance)
KERNELS = {"k_proj_reduce<8>": "_ZN3s4b13k_proj_reduceILi8EE", "k_proj_reduce<16>": "_ZN3s4b13k_proj_reduceILi16EE", "k_proj_reduce<32>": "_ZN3s4b13k_proj_reduceILi32EE",
           "k_proj_fold": "_ZN3s4b11k_proj_foldE", "k_proj_solve": "_ZN3s4b12k_proj_solveE"}
NO_LDS = [k for k in KERNELS if k != "k_proj_solve"]


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
    assert len([b for b in blocks if b.split()[0].startswith("_ZN3s4b13k_proj_reduceILi")]) == 3, "k_proj_reduce has other instances than 8, 16 and 32"
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
def test_projection_kernels_use_no_private_memory(usage, kernel):
    u = usage[kernel]
    print(f"{kernel}: {u}")
    assert u["spill"] == 0 and u["scratch"] == 0, f"{kernel} uses private memory: {u}"
    if kernel in NO_LDS:
        assert u["lds"] == 0, u


def test_projection_kernels_are_included_after_the_level_kernels():
    src = open(os.path.join(CSRC, "dev_hip.hip")).read()
    assert '#include "dev_groups.inc"\n#include "readout_projection.inc"\n' in src
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "readout_projection.inc" in mk and mk.count("CXXFLAGS ?=") == 1
    text = open(os.path.join(CSRC, "readout_projection.inc")).read()
    assert not re.search(r"\w*[aA]tomic\w*\s*\(", text), "readout_projection.inc calls an atomic function"
    for k in ("k_proj_reduce", "k_proj_fold", "k_proj_solve"):
        assert f"void {k}(" in text
    # the value kernels of either arm, the chunk rule and the sort (k_row_quantiles) are called through the shared helpers; k_level_rows is launched here
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    for used in ("chunk_plan(", "chunk_grid(", "arm_values_prepare(", "arm_values_launch(", "LevelsSummary sum;", "sum.prepare(", "sum.run(",
                 "hipLaunchKernelGGL(k_level_rows, "):
        assert used in code, used
    # the summary kernels are used, not copied
    assert "void k_level_rows(" not in text and "void k_row_quantiles(" not in text
