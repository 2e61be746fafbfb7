"""Guard of the register allocation of the read-out kernels of the kept trees (stan4bart_amd/csrc/dev_readout.inc and the three files that use it),
compile only: hipcc cross-compiles gfx950 without a GPU.  With the mechanics of tests/test_kernel_resources.py the main translation unit is compiled
ONCE for the device alone with the product's CXXFLAGS and `-Rpass-analysis=kernel-resource-usage` is read.

The walking kernels — k_predict_summary, k_partial_dependence, k_predict_values, each <staged / global> — run workgroups of 1 024 threads, four waves
per SIMD: more than 128 VGPRs and a kernel cannot be launched at all, and a spill is paid once per tree step (in k_partial_dependence G x (affected
trees) times per (row, draw)).  k_predict_summary<staged> measures 125 VGPRs with erfc inline.  The first build of
k_partial_dependence did spill (8 VGPRs, 36 bytes of scratch on the staged route): erfc inlined into the grid loop had its polynomial constants
hoisted into some sixty registers for the whole kernel.  Phi is therefore an out-of-line function there and in k_predict_values (readout_phi), and
those kernels measure 75 / 63 and 69 / 64 VGPRs — DESIGN.md 5.6, 5.7.  k_row_quantiles sorts in LDS: no private memory either."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stan4bart_amd", "csrc")

# (mangled: s4b::k_predict_summary<STAGED>(SummaryDev), s4b::k_partial_dependence<STAGED>(PdDev), s4b::k_predict_values<STAGED>(QuantileDev),
# s4b::k_row_quantiles(QuantileDev))
KERNELS = {("summary", "staged"): "_ZN3s4b17k_predict_summaryILb1EEE", ("summary", "global"): "_ZN3s4b17k_predict_summaryILb0EEE",
           ("pd", "staged"): "_ZN3s4b20k_partial_dependenceILb1EEE", ("pd", "global"): "_ZN3s4b20k_partial_dependenceILb0EEE",
           ("values", "staged"): "_ZN3s4b16k_predict_valuesILb1EEE", ("values", "global"): "_ZN3s4b16k_predict_valuesILb0EEE",
           ("sort", None): "_ZN3s4b15k_row_quantilesE"}


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


def _fits_a_1024_thread_workgroup(name, u):
    assert u["spill"] == 0 and u["scratch"] == 0, f"{name} uses private memory: {u['vgprs']} VGPRs, occupancy {u['occupancy']} waves/SIMD: {u}"
    # a workgroup is 16 waves, four per SIMD: more than 128 VGPRs and it cannot be launched at all
    assert u["vgprs"] <= 128 and u["occupancy"] >= 4, f"{name}: {u['vgprs']} VGPRs, occupancy {u['occupancy']} waves/SIMD: {u}"
    assert u["lds"] == 0, (name, u)          # all LDS is dynamic: the host sizes it per call (readout_plan)


@pytest.mark.parametrize("key", ["staged", "global"])
def test_summary_kernels_fit_a_1024_thread_workgroup_without_private_memory(usage, key):
    _fits_a_1024_thread_workgroup(f"k_predict_summary<{key}>", usage["summary", key])


def test_partial_dependence_kernels_use_no_private_memory(usage):
    for key in ("staged", "global"):
        _fits_a_1024_thread_workgroup(f"k_partial_dependence<{key}>", usage["pd", key])


@pytest.mark.parametrize("key", ["staged", "global"])
def test_value_kernels_fit_a_1024_thread_workgroup_without_private_memory(usage, key):
    _fits_a_1024_thread_workgroup(f"k_predict_values<{key}>", usage["values", key])


def test_sort_kernel_uses_no_private_memory(usage):
    u = usage["sort", None]
    assert u["spill"] == 0 and u["scratch"] == 0, f"k_row_quantiles uses private memory: {u}"
    assert u["lds"] == 0, u                 # dynamic: 8 x max(padded draws, 4096) bytes


def test_the_chunk_rule_and_the_value_launches_are_written_once():
    """The host side of a chunked read-out: rows per chunk, segments of draws and the launches of the two value kernels stand in the file
    that owns the kernel and nowhere else under csrc — a read-out calls chunk_plan, chunk_grid and the launch helpers.  Source text with the comments
    stripped; nothing is compiled."""
    code = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".inc", ".hip", ".hpp")):
            with open(os.path.join(CSRC, name)) as f:
                code[name] = "\n".join(line.split("//")[0] for line in f.read().splitlines())

    def files_with(pattern):
        return sorted(n for n, c in code.items() if re.search(pattern, c))

    # the deciding expressions of the rule: the filling of the device, the least segment, the scratch over 8 bytes per value, whole multiples of rows
    for pattern in (r"\bQT_FILL\b", r"\bQT_SEG_MIN\b", r"scratch / \(8 \*", r"/ multiple \* multiple\b", r"scratchBytes > 0 \?"):
        assert files_with(pattern) == ["dev_quantile.inc"], (pattern, files_with(pattern))
    q = code["dev_quantile.inc"]
    assert len(re.findall(r"scratch / \(8 \*", q)) == 1 and len(re.findall(r"\bQT_SEG_MIN\b", q)) == 2 and len(re.findall(r"\bQT_FILL\b", q)) == 2          # the constant and its one use
    assert "scratch / (8 * S * perRowDraw) / multiple * multiple" in q
    # the launches of the value kernels
    assert files_with(r"hipLaunchKernelGGL\(k_predict_values<") == ["dev_quantile.inc"]
    assert files_with(r"hipLaunchKernelGGL\(k_contrast_values<") == ["dev_contrast.inc"]
    assert len(re.findall(r"hipLaunchKernelGGL\(k_predict_values<", q)) == 2 and len(re.findall(r"hipLaunchKernelGGL\(k_contrast_values<", code["dev_contrast.inc"])) == 2
