"""Guard of the register allocation of the check kernels (stan4bart_amd/csrc/readout_check.inc), compile only, with the mechanics of
tests/test_spread_kernel_resources.py: the main translation unit is compiled once for the device alone with the product's CXXFLAGS and
`-Rpass-analysis=kernel-resource-usage` is read.

k_check_reduce forms a Philox block, Box-Muller (or two erfc and two logarithms) and the replicate per row beside four rows in flight and eleven
running statistics per lane; a spill — of a vector register to scratch or of a scalar register into vector lanes — would be paid per row of every slab: neither
is allowed in any instance.  Its weight histogram lives in DYNAMIC LDS, (T + 1) x 512 bytes sized at
launch, so the static LDS of every instance is 0; the instances without thresholds use no LDS at all.  The bin route is a template parameter, as in
k_spread_reduce (four instances).  k_check_fold keeps the partials of eight slabs
in flight, k_check_finish a handful of sums.  The vector registers and the occupancy are printed, not asserted."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stan4bart_amd", "csrc")

# (mangled prefixes, one per instance: <LINK, BINS, SEARCH>)
KERNELS = {"k_check_reduce<0, false, false>": "_ZN3s4b14k_check_reduceILi0ELb0ELb0EE", "k_check_reduce<0, true, false>": "_ZN3s4b14k_check_reduceILi0ELb1ELb0EE",
           "k_check_reduce<0, true, true>": "_ZN3s4b14k_check_reduceILi0ELb1ELb1EE", "k_check_reduce<1, false, false>": "_ZN3s4b14k_check_reduceILi1ELb0ELb0EE",
           "k_check_fold": "_ZN3s4b12k_check_foldE",
           "k_check_finish": "_ZN3s4b14k_check_finishE"}


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
    assert len([b for b in blocks if b.split()[0].startswith("_ZN3s4b14k_check_reduceIL")]) == 4, "k_check_reduce has other instances than the four in use"
    found = {}
    for key, prefix in KERNELS.items():
        hit = [b for b in blocks if b.split()[0].startswith(prefix)]
        assert len(hit) == 1, (key, [b.split()[0] for b in blocks])

        def field(name, text=hit[0]):
            return int(re.search(name + r": (\d+)", text).group(1))
        found[key] = dict(vgprs=field("VGPRs"), spill=field("VGPRs Spill"), sgpr_spill=field("SGPRs Spill"), scratch=field(r"ScratchSize \[bytes/lane\]"),
                          occupancy=field(r"Occupancy \[waves/SIMD\]"), lds=field(r"LDS Size \[bytes/block\]"))
    return found


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_check_kernels_use_no_private_memory(usage, kernel):
    u = usage[kernel]
    print(f"{kernel}: {u}")
    assert u["spill"] == 0 and u["scratch"] == 0, f"{kernel} uses private memory: {u}"
    assert u["sgpr_spill"] == 0, f"{kernel} spills scalar registers into vector lanes: {u}"
    assert u["lds"] == 0, f"{kernel} has static LDS (the weight histogram is dynamic, sized by T at launch): {u}"


def test_check_kernels_are_included_after_the_spread_kernels_and_share_their_routines():
    src = open(os.path.join(CSRC, "dev_hip.hip")).read()
    assert '#include "readout_spread.inc"\n#include "readout_check.inc"\n' in src
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "readout_check.inc" in mk and mk.count("CXXFLAGS ?=") == 1
    text = open(os.path.join(CSRC, "readout_check.inc")).read()
    assert not re.search(r"\w*[aA]tomic\w*\s*\(", text), "readout_check.inc calls an atomic function"
    for k in ("k_check_reduce", "k_check_fold", "k_check_finish"):
        assert f"void {k}(" in text
    # the value kernel, the chunk rule and the summary over the draws (k_level_rows, k_row_quantiles) are called through the shared helpers
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    for used in ("chunk_plan(", "chunk_grid(", "predict_values_prepare(", "predict_values_launch(", "LevelsSummary sum;", "sum.prepare(", "sum.run("):
        assert used in code, used
    # the value kernel, the summary kernels and the bin routine are used, not copied
    assert "void k_level_rows(" not in text and "void k_row_quantiles(" not in text and "void k_predict_values(" not in text
    assert "sp_bins<SEARCH, CK_AHEAD>(" in text and "void sp_bins(" not in text
    spread = open(os.path.join(CSRC, "readout_spread.inc")).read()
    assert spread.count("void sp_bins(") == 1 and "sp_bins<SEARCH, SP_AHEAD>(" in spread
    assert "philox_normal(" in text and "philox_uniform(" in text and "readout_phi(" in text
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in text and "extern __shared__" in text
    # the stated order is written once and run by the kernels and by the host's statistics of y
    for f in ("ck_add", "ck_partial", "ck_combine"):
        assert text.count(f"__host__ __device__ __forceinline__ void {f}(") == 1 and text.count(f"{f}(") >= 3, f
