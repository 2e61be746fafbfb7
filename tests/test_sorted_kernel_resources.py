"""Guard of the register allocation of the selection kernels (stan4bart_amd/csrc/readout_sorted.inc), compile only, with the mechanics of
tests/test_describe_kernel_resources.py: the main translation unit is compiled once for the device alone with the product's CXXFLAGS and
`-Rpass-analysis=kernel-resource-usage` is read.

k_sorted_hist (every instantiation), k_sorted_scan, k_sorted_count and k_sorted_finish use no private memory, spill no vector or scalar register and
hold 0 bytes of static LDS (the counting tables, the scan's scratch and the cuts are dynamic LDS).  The value kernels, the summary over the draws and
the monotone key are the family's, called and not copied.  Every atomic of the source adds integers.  The vector registers and the occupancy are
printed, not asserted.  Only the resource remarks and the source text are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stan4bart_amd", "csrc")
KERNELS = ("k_sorted_hist", "k_sorted_scan", "k_sorted_count", "k_sorted_finish")


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
    for b in blocks:
        name = b.split()[0]
        for k in KERNELS:
            if re.match(r"_ZN3s4b\d+" + k + r"(E|I)", name):
                def field(what, text=b):
                    return int(re.search(what + r": (\d+)", text).group(1))
                found.setdefault(k, []).append(dict(name=name, vgprs=field("VGPRs"), sgprs=field("SGPRs"), spill=field("VGPRs Spill"),
                                                    sgpr_spill=field("SGPRs Spill"), scratch=field(r"ScratchSize \[bytes/lane\]"),
                                                    occupancy=field(r"Occupancy \[waves/SIMD\]"), lds=field(r"LDS Size \[bytes/block\]")))
    return found


def test_selection_kernels_use_no_private_memory(usage):
    assert sorted(usage) == sorted(KERNELS), sorted(usage)
    assert len(usage["k_sorted_hist"]) == 3, "k_sorted_hist for 8, 4 and 2 draws per workgroup"
    for k in KERNELS:
        for u in usage[k]:
            print(f"{k}: {u}")
            assert u["spill"] == 0 and u["scratch"] == 0, f"{k} uses private memory: {u}"
            assert u["sgpr_spill"] == 0, f"{k} spills scalar registers into vector lanes: {u}"
            assert u["lds"] == 0, f"{k}: static LDS {u}"


def test_selection_kernels_are_included_behind_describe_and_share_the_family_routines():
    src = open(os.path.join(CSRC, "dev_hip.hip")).read()
    assert '#include "readout_describe.inc"\n#include "readout_sorted.inc"\n' in src
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "readout_sorted.inc" in mk and mk.count("CXXFLAGS ?=") == 1
    text = open(os.path.join(CSRC, "readout_sorted.inc")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    for k in KERNELS:
        assert len(re.findall(r"void " + k + r"\(", code)) == 1, k
    assert "__shared__ " not in code.replace("extern __shared__ ", ""), "static LDS"
    for used in ("arm_values_launch(", "arm_values_prepare(", "chunk_grid(", "readout_plan(", "LevelsSummary", "qt_key(", "qt_value(", "contrast_upload("):
        assert used in code, used
    for defined in ("k_predict_values", "k_contrast_values", "k_level_rows", "k_row_quantiles", "qt_key"):
        assert not re.search(r"\b(void|uint64_t|double)\s+" + defined + r"\s*\(", text), defined
    assert "walk_trees" not in code and "walk_all" not in code, "the trees are walked by the value kernels alone"
    assert "asm" not in code


def test_every_atomic_adds_integers():
    text = open(os.path.join(CSRC, "readout_sorted.inc")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    atomics = re.findall(r"atomic\w*", code, re.I)
    assert atomics and set(atomics) == {"atomicAdd"}, atomics
    # every atomicAdd targets the uint32 tables: &tab[...] in LDS (uint32_t* tab) or &dst[...] in global memory (uint32_t* dst)
    targets = re.findall(r"atomicAdd\(&(\w+)\[", code)
    assert len(targets) == len(atomics) and set(targets) == {"tab", "dst"}, targets
    assert re.search(r"uint32_t\* tab\b", code) and re.search(r"uint32_t\* dst = a\.hist\b", code) and re.search(r"uint32_t\* hist;", code)
    for name in ("atomicAdd_system", "unsafeAtomicAdd", "atomicMax", "atomicMin", "atomicCAS", "atomicExch"):
        assert name not in code, name
