"""Guard of the register allocation of the describe kernel (stan4bart_amd/csrc/readout_describe.inc), compile only, with the mechanics of
tests/test_curve_kernel_resources.py: the main translation unit is compiled once for the device alone with the product's CXXFLAGS and
`-Rpass-analysis=kernel-resource-usage` is read.

k_row_describe holds its rows as keys in dynamic LDS (the sort's bytes + 8 R) and nothing else: no private memory, no spilled vector or scalar
register, 0 bytes of static LDS, no atomics.  The sort and the type-7 read are dev_quantile.inc's, called and not copied.  The vector registers and the
occupancy are printed, not asserted."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stan4bart_amd", "csrc")
PREFIX = "_ZN3s4b14k_row_describeE"


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
    hit = [b for b in blocks if b.split()[0].startswith(PREFIX)]
    assert len(hit) == 1, [b.split()[0] for b in blocks if "describe" in b.split()[0]]

    def field(name):
        return int(re.search(name + r": (\d+)", hit[0]).group(1))
    return dict(vgprs=field("VGPRs"), sgprs=field("SGPRs"), spill=field("VGPRs Spill"), sgpr_spill=field("SGPRs Spill"),
                scratch=field(r"ScratchSize \[bytes/lane\]"), occupancy=field(r"Occupancy \[waves/SIMD\]"), lds=field(r"LDS Size \[bytes/block\]"))


def test_describe_kernel_uses_no_private_memory(usage):
    print(f"k_row_describe: {usage}")
    assert usage["spill"] == 0 and usage["scratch"] == 0, f"k_row_describe uses private memory: {usage}"
    assert usage["sgpr_spill"] == 0, f"k_row_describe spills scalar registers into vector lanes: {usage}"
    assert usage["lds"] == 0, f"k_row_describe: static LDS {usage}"


def test_describe_kernel_is_included_behind_the_curves_and_shares_the_family_routines():
    src = open(os.path.join(CSRC, "dev_hip.hip")).read()
    assert '#include "readout_curves.inc"\n#include "readout_describe.inc"\n' in src
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "readout_describe.inc" in mk and mk.count("CXXFLAGS ?=") == 1
    text = open(os.path.join(CSRC, "readout_describe.inc")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert text.count("void k_row_describe(") == 1
    assert not re.search(r"atomic", code, re.I), "the describe kernel and its host side use no atomics"
    assert "__shared__ " not in code.replace("extern __shared__ ", ""), "static LDS"
    # the sort, the type-7 read, the chunk plan and the value launches are used, not copied
    for used in ("qt_sort_rows(", "qt_type7_rows(", "chunk_plan(", "arm_values_launch(", "arm_values_prepare(", "readout_plan(", "chunk_grid(", "wave_argmin("):
        assert used in code, used
    assert code.count("qt_sort_rows(key, N, Sp)") == 2, "the sort runs once for the row and once more for the deviations"
    for copied in ("void qt_sort_rows(", "void k_row_quantiles(", "void qt_type7_rows(", "void k_predict_values(", "void k_contrast_values("):
        assert copied not in text, copied
    wave = open(os.path.join(CSRC, "dev_wave.hpp")).read()
    assert wave.count("void wave_argmin(") == 1 and wave.index("double wave_min(") < wave.index("void wave_argmin(")
