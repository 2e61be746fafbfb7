"""Guard of the register allocation of the contrast kernels (stan4bart_amd/csrc/dev_contrast.inc), compile only, with the mechanics of
tests/test_readout_kernel_resources.py: the main translation unit is compiled once for the device alone with the product's CXXFLAGS and
`-Rpass-analysis=kernel-resource-usage` is read.

k_contrast_values<staged / global> runs workgroups of 1 024 threads, four waves per SIMD: more than 128 VGPRs and it cannot be launched at all, and a
spill is paid once per tree step of both arms.  It holds k_partial_dependence's walk of four chains, the group of QT_GROUP values of k_predict_values
and the two arms' sums; Phi stays out of line (readout_phi).  The first build measures 95 / 83 VGPRs, no spill, no scratch.
k_contrast_reduce keeps eight weighted sums per thread in registers: no private memory."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stan4bart_amd", "csrc")

# (mangled: s4b::k_contrast_values<STAGED>(ContrastDev), s4b::k_contrast_reduce(ContrastDev))
KERNELS = {("values", "staged"): "_ZN3s4b17k_contrast_valuesILb1EEE", ("values", "global"): "_ZN3s4b17k_contrast_valuesILb0EEE",
           ("reduce", None): "_ZN3s4b17k_contrast_reduceE"}


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
    res = {}
    for key, prefix in KERNELS.items():
        hit = [b for b in blocks if b.split()[0].startswith(prefix)]
        assert len(hit) == 1, (key, [b.split()[0] for b in blocks])

        def field(name, text=hit[0]):
            return int(re.search(name + r": (\d+)", text).group(1))
        res[key] = dict(vgprs=field("VGPRs"), spill=field("VGPRs Spill"), scratch=field(r"ScratchSize \[bytes/lane\]"),
                        occupancy=field(r"Occupancy \[waves/SIMD\]"), lds=field(r"LDS Size \[bytes/block\]"))
    return res


@pytest.mark.parametrize("key", ["staged", "global"])
def test_value_kernels_fit_a_1024_thread_workgroup_without_private_memory(usage, key):
    u = usage["values", key]
    name = f"k_contrast_values<{key}>"
    assert u["spill"] == 0 and u["scratch"] == 0, f"{name} uses private memory: {u}"
    # a workgroup is 16 waves, four per SIMD: more than 128 VGPRs and it cannot be launched at all
    assert u["vgprs"] <= 128 and u["occupancy"] >= 4, f"{name}: {u['vgprs']} VGPRs, occupancy {u['occupancy']} waves/SIMD: {u}"
    assert u["lds"] == 0, (name, u)          # all LDS is dynamic: the host sizes it per call (readout_plan)


def test_reduce_kernel_uses_no_private_memory(usage):
    u = usage["reduce", None]
    assert u["spill"] == 0 and u["scratch"] == 0, f"k_contrast_reduce uses private memory: {u}"
    assert u["lds"] == 0, u
