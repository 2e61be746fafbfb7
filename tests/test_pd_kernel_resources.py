"""Guard of k_partial_dependence's register allocation (compile only: hipcc cross-compiles gfx950 without a GPU), with the mechanics of
tests/test_kernel_resources.py: the main translation unit is compiled for the device alone with the product's CXXFLAGS and
`-Rpass-analysis=kernel-resource-usage` is read.

Both instantiations (staged, global) must use no private memory: a thread keeps four walks in flight in the loop over the grid points, and a spill
there is paid G x (affected trees) times per (row, draw).  The first build of the kernel did spill (8 VGPRs, 36 bytes of scratch on the staged
route): erfc inlined into the grid loop had its polynomial constants hoisted into some sixty registers for the whole kernel.  Phi is therefore an
out-of-line function (pd_phi), and the kernels measure 75 (staged) and 63 (global) VGPRs — DESIGN.md 5.6."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stan4bart_amd", "csrc")


def _pd_usage():
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
    for staged in (1, 0):          # (mangled: s4b::k_partial_dependence<STAGED>)
        hit = [b for b in blocks if b.split()[0].startswith("_ZN3s4b20k_partial_dependenceILb%dEEE" % staged)]
        assert len(hit) == 1, (staged, [b.split()[0] for b in blocks])

        def field(name, text=hit[0]):
            return int(re.search(name + r": (\d+)", text).group(1))
        res["staged" if staged else "global"] = dict(vgprs=field("VGPRs"), spill=field("VGPRs Spill"), scratch=field(r"ScratchSize \[bytes/lane\]"),
                                                     occupancy=field(r"Occupancy \[waves/SIMD\]"), lds=field(r"LDS Size \[bytes/block\]"))
    return res


def test_partial_dependence_kernels_use_no_private_memory():
    res = _pd_usage()
    assert set(res) == {"staged", "global"}
    for key, u in res.items():
        assert u["spill"] == 0 and u["scratch"] == 0, f"k_partial_dependence<{key}> uses private memory: {u['vgprs']} VGPRs, occupancy {u['occupancy']} waves/SIMD: {u}"
        # a workgroup is 16 waves, four per SIMD: more than 128 VGPRs and it cannot be launched at all
        assert u["vgprs"] <= 128 and u["occupancy"] >= 4, f"k_partial_dependence<{key}>: {u['vgprs']} VGPRs, occupancy {u['occupancy']} waves/SIMD: {u}"
        assert u["lds"] == 0, (key, u)          # all LDS is dynamic: the host sizes it per call (pd_lds_bytes)
