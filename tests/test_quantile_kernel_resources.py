"""Guard of the register allocation of s4b_predict_quantiles' kernels (compile only: hipcc cross-compiles gfx950 without a GPU), with the mechanics
of tests/test_pd_kernel_resources.py: the main translation unit is compiled for the device alone with the product's CXXFLAGS and
`-Rpass-analysis=kernel-resource-usage` is read.

k_predict_values<staged / global> is k_predict_summary's walk with a group of QT_GROUP draws buffered in registers in place of the Welford pair: a
workgroup is 1 024 threads, four waves per SIMD, so more than 128 VGPRs and it cannot be launched at all, and a spill is paid once per tree step.
k_row_quantiles sorts in LDS: no private memory either.  The numbers are in DESIGN.md 5.7."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stan4bart_amd", "csrc")


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
    # (mangled: s4b::k_predict_values<STAGED>(QuantileDev), s4b::k_row_quantiles(QuantileDev))
    for key, prefix in (("staged", "_ZN3s4b16k_predict_valuesILb1EEE"), ("global", "_ZN3s4b16k_predict_valuesILb0EEE"), ("sort", "_ZN3s4b15k_row_quantilesE")):
        hit = [b for b in blocks if b.split()[0].startswith(prefix)]
        assert len(hit) == 1, (key, [b.split()[0] for b in blocks])

        def field(name, text=hit[0]):
            return int(re.search(name + r": (\d+)", text).group(1))
        res[key] = dict(vgprs=field("VGPRs"), spill=field("VGPRs Spill"), scratch=field(r"ScratchSize \[bytes/lane\]"),
                        occupancy=field(r"Occupancy \[waves/SIMD\]"), lds=field(r"LDS Size \[bytes/block\]"))
    return res


@pytest.mark.parametrize("key", ["staged", "global"])
def test_value_kernels_fit_a_1024_thread_workgroup_without_private_memory(usage, key):
    u = usage[key]
    assert u["spill"] == 0 and u["scratch"] == 0, f"k_predict_values<{key}> uses private memory: {u}"
    assert u["vgprs"] <= 128 and u["occupancy"] >= 4, f"k_predict_values<{key}>: {u['vgprs']} VGPRs, occupancy {u['occupancy']} waves/SIMD: {u}"
    assert u["lds"] == 0, (key, u)          # all LDS is dynamic: the host sizes it per call (quantile_lds_bytes)


def test_sort_kernel_uses_no_private_memory(usage):
    u = usage["sort"]
    assert u["spill"] == 0 and u["scratch"] == 0, f"k_row_quantiles uses private memory: {u}"
    assert u["lds"] == 0, u                 # dynamic: 8 x max(padded draws, 4096) bytes
