"""Guard of the register allocation of k_chain_rows (stan4bart_amd/csrc/dev_conv.inc), compile only, with the mechanics of
tests/test_loo_kernel_resources.py: the main translation unit is compiled once for the device alone with the product's CXXFLAGS and
`-Rpass-analysis=kernel-resource-usage` is read.

k_chain_rows holds the log-likelihood of quantity 1 (log, exp of the device library inlined; Phi stays out of line, readout_phi), the chain sums and, in
its inner loop, four partial lag sums beside the running pair state.  A spill would be paid per product of every lag: no spill, no private memory.
All its LDS is dynamic (8 max(padded draws, 4096) + 128 + 16 (rows in flight) (chains) + 2048 (rows in flight) bytes: DESIGN.md 5.11).  A workgroup
is four waves, one per SIMD, so any register count can be launched: the occupancy is printed, not asserted."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stan4bart_amd", "csrc")

KERNEL = "_ZN3s4b12k_chain_rowsE"          # (mangled: s4b::k_chain_rows(ConvDev))


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
    hit = [b for b in blocks if b.split()[0].startswith(KERNEL)]
    assert len(hit) == 1, [b.split()[0] for b in blocks]

    def field(name):
        return int(re.search(name + r": (\d+)", hit[0]).group(1))
    return dict(vgprs=field("VGPRs"), spill=field("VGPRs Spill"), scratch=field(r"ScratchSize \[bytes/lane\]"),
                occupancy=field(r"Occupancy \[waves/SIMD\]"), lds=field(r"LDS Size \[bytes/block\]"))


def test_row_kernel_uses_no_private_memory(usage):
    print(f"k_chain_rows: {usage}")
    assert usage["spill"] == 0 and usage["scratch"] == 0, f"k_chain_rows uses private memory: {usage}"
    assert usage["lds"] == 0, usage          # dynamic: the host sizes it per call


def test_row_kernel_is_part_of_the_main_unit_after_the_loo_kernel():
    src = open(os.path.join(CSRC, "dev_hip.hip")).read()
    assert '#include "dev_loo.inc"\n#include "dev_conv.inc"\n' in src
    conv = open(os.path.join(CSRC, "dev_conv.inc")).read()
    body = conv.split("struct ConvDev")[1]
    assert "ppd_loglik(" in body and "atomic" not in body and "qt_sort_rows" not in body and "erfc" not in conv
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "dev_conv.inc" in mk and mk.count("CXXFLAGS ?=") == 1
