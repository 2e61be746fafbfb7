"""Guard of the batched sweep kernels' register allocation (compile only, like tests/test_kernel_resources.py): k_sbatch* run the body of
the kernel each one batches and must fit the same budget — eight waves of one workgroup per CU, no spills — with the same LDS."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stan4bart_amd", "csrc")
PAIRS = (("8k_sbatchE", "7k_sweepE"), ("12k_sbatch_fewE", "11k_sweep_fewE"), ("11k_sbatch_spE", "10k_sweep_spE"),
         ("15k_sbatch_few_spE", "14k_sweep_few_spE"), ("10k_sbatch_wE", "9k_sweep_wE"))


def test_batched_sweep_kernels_fit_the_budget_of_the_kernels_they_batch():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not found")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    cxx = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).split()
    swp = re.search(r"^SWEEPFLAGS \?= (.*)$", mk, re.M).group(1).split()
    cmd = [hipcc, "--offload-arch=gfx950", *cxx, *swp, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, "dev_sweep.hip"]
    out = subprocess.run(cmd, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", out.stdout)[1:]

    def usage(mangled):
        hit = [b for b in blocks if mangled in b.split()[0]]
        assert len(hit) == 1, (mangled, [b.split()[0] for b in blocks])

        def field(name):
            return int(re.search(name + r": (\d+)", hit[0]).group(1))
        return dict(vgprs=field("VGPRs"), spill=field("VGPRs Spill"), scratch=field(r"ScratchSize \[bytes/lane\]"),
                    occupancy=field(r"Occupancy \[waves/SIMD\]"), lds=field(r"LDS Size \[bytes/block\]"))
    for batched, single in PAIRS:
        b, s = usage(batched), usage(single)
        assert b["vgprs"] <= 256 and b["occupancy"] >= 2 and b["spill"] <= 2 and b["scratch"] <= 1880, (batched, b)
        assert b["lds"] == s["lds"], (batched, b, single, s)
