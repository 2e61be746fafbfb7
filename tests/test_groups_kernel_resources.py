"""Guard of the register allocation of the level kernels (stan4bart_amd/csrc/dev_groups.inc), compile only, with the mechanics of
tests/test_convergence_kernel_resources.py: the main translation unit is compiled once for the device alone with the product's CXXFLAGS and
`-Rpass-analysis=kernel-resource-usage` is read.

k_level_reduce keeps one partial sum, the current label and a few pointers per thread, k_level_fold one sum, k_level_rows three: none of them has a
reason to touch private memory, and a spill would be paid per row of every slab.  None uses LDS.  The occupancy is printed, not asserted."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stan4bart_amd", "csrc")

KERNELS = {"k_level_reduce": "_ZN3s4b14k_level_reduceE", "k_level_fold": "_ZN3s4b12k_level_foldE", "k_level_rows": "_ZN3s4b12k_level_rowsE"}          # (mangled prefixes)


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
def test_level_kernels_use_no_private_memory(usage, kernel):
    u = usage[kernel]
    print(f"{kernel}: {u}")
    assert u["spill"] == 0 and u["scratch"] == 0, f"{kernel} uses private memory: {u}"
    assert u["lds"] == 0, u


def test_level_kernels_are_the_last_include_of_the_main_unit():
    src = open(os.path.join(CSRC, "dev_hip.hip")).read()
    assert '#include "dev_conv.inc"\n#include "dev_contrast.inc"\n#include "dev_groups.inc"\n' in src
    after = src.split('#include "dev_groups.inc"\n')[1]
    assert not re.search(r'#include "dev_\w+\.inc"', after), "dev_groups.inc is not the last of the kernel includes"
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "dev_groups.inc" in mk and mk.count("CXXFLAGS ?=") == 1
    text = open(os.path.join(CSRC, "dev_groups.inc")).read()
    assert not re.search(r"\w*[aA]tomic\w*\s*\(", text), "dev_groups.inc calls an atomic function"
    for k in KERNELS:
        assert f"void {k}(" in text
    # the value kernels of either arm, the chunk rule and the sort (k_row_quantiles) are called through the shared helpers
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    for used in ("chunk_plan(", "chunk_grid(", "arm_values_prepare(", "arm_values_launch(", "row_quantiles_prepare(", "row_quantiles_launch(", "sum.prepare(", "sum.run("):
        assert used in code, used
    assert "qt_sort_rows" not in text
