"""Latent mode "parallel" (bart_args latents, s4b_set_latent_mode 1) where no GPU is needed: the refusals, the Philox4x32-10 generator against
the published Random123 known-answer vectors, the truncated-normal sampler of the same header on the host, and the register budget of the new
kernel (compile only).  The draws through a real sampler: tests/test_gpu_latents_parallel.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import make_sampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stan4bart_amd", "csrc")


def _data(n=80, seed=3, binary=True):
    g = np.random.default_rng(seed)
    xb = g.random((n, 4))
    X = g.random((n, 1))
    eta = 2.0 * (xb[:, 0] - 0.5) + X[:, 0] + 0.5 * g.standard_normal(n)
    y = (eta > 0.0).astype(np.float64) if binary else eta
    return y, xb, X


def _args(binary=True, **bart):
    from stan4bart_amd import make_sampler_args
    y, xb, X = _data(binary=binary)
    return make_sampler_args(y, xb, X=X, family="binomial" if binary else "gaussian", iter=4, warmup=2,
                             bart_args={"n.trees": 5, **bart})


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------

def test_latents_option_is_validated():
    assert _args().latents == "exact"
    assert _args(latents="exact").latents == "exact"
    assert _args(latents="parallel").latents == "parallel"
    with pytest.raises(ValueError, match="latents"):
        _args(latents="bogus")
    with pytest.raises(ValueError, match="binary response"):
        _args(binary=False, latents="parallel")


def test_stan4bart_refuses_a_bad_latents_value(emul_lib):
    from stan4bart_amd import stan4bart
    from stan4bart_amd.abi import Sampler
    y, xb, X = _data()
    for bad, fam in (("bogus", "binomial"), ("parallel", "gaussian")):
        with pytest.raises(ValueError, match="latents"):
            stan4bart(y if fam == "binomial" else xb[:, 0], xb, X=X, family=fam, chains=1, seed=1, iter=4, warmup=2,
                      bart_args={"n.trees": 5, "latents": bad}, make_sampler=lambda a, st: Sampler(emul_lib, "emu_", a, st))


def test_emulated_device_layer_refuses_the_parallel_draw(emul_lib):
    """tests/emul's device layer has no parallel draw: the setter says so and the sampler stays in the exact mode (it never runs the exact draw
    in place of the requested one)."""
    s = make_sampler(emul_lib, "emu_", _args())
    try:
        assert s.get_latent_mode() == 0
        with pytest.raises(RuntimeError, match="device layer has no parallel latent draw"):
            s.set_latent_mode(1)
        assert s.get_latent_mode() == 0
        s.set_latent_mode(0)
        with pytest.raises(RuntimeError, match="latent mode must be 0"):
            s.set_latent_mode(2)
    finally:
        s.free()
    with pytest.raises(RuntimeError, match="device layer has no parallel latent draw"):
        make_sampler(emul_lib, "emu_", _args(latents="parallel"))


def test_parallel_mode_is_refused_for_a_continuous_response(emul_lib):
    s = make_sampler(emul_lib, "emu_", _args(binary=False))
    try:
        with pytest.raises(RuntimeError, match="continuous"):
            s.set_latent_mode(1)
        assert s.get_latent_mode() == 0
    finally:
        s.free()


def test_exact_mode_state_blob_is_unchanged(emul_lib):
    """The exact mode's state carries no latent fields: header reserved[1] = 0 and no tail (the layout conftest.StateView parses)."""
    from conftest import StateView
    s = make_sampler(emul_lib, "emu_", _args())
    try:
        s.run(2, True)
        blob = s.get_state()
        StateView(blob)                                   # asserts that the layout ends where it always did
        assert np.frombuffer(blob, dtype=np.int64, count=1, offset=40)[0] == 0
    finally:
        s.free()


# ---- the generator and the sampler on the host ---------------------------------------------------------------------------------------------------

def _compile(tmp_path, src, name):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    f = tmp_path / (name + ".cpp")
    f.write_text(src)
    exe = tmp_path / name
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", CSRC, "-o", str(exe), str(f)], check=True)
    return str(exe)


# Random123 kat_vectors: philox4x32 10 <counter> <key> <expected>
KAT = [((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox4x32_10_known_answers(tmp_path):
    exe = _compile(tmp_path, """
#include "philox.hpp"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
  s4b::Philox4 c; for (int i = 0; i < 4; ++i) c.v[i] = (uint32_t)strtoul(argv[1 + i], nullptr, 0);
  const s4b::Philox4 r = s4b::philox4x32_10(c, (uint32_t)strtoul(argv[5], nullptr, 0), (uint32_t)strtoul(argv[6], nullptr, 0));
  printf("%u %u %u %u\\n", r.v[0], r.v[1], r.v[2], r.v[3]);
}
""", "kat")
    for ctr, key, want in KAT:
        out = subprocess.run([exe, *map(str, ctr), *map(str, key)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
        assert tuple(int(v) for v in out) == want, (ctr, key, out)


def test_host_truncated_normal_is_exact(tmp_path):
    """philox_trunc_normal, the device's sampler compiled for the host: 40 000 draws per bound, both branches (normal rejection below 0,
    Robert's exponential proposal from 0 on), bounds up to 40 (|mean| = 40 occurs early in chains): KS against the truncated normal, computed
    with log survival functions so that the far tail is not 1 - Phi."""
    from scipy import stats
    exe = _compile(tmp_path, """
#include "philox.hpp"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
  const double lower = atof(argv[1]); const int m = atoi(argv[2]);
  for (int j = 0; j < m; ++j) {
    double x; if (!s4b::philox_trunc_normal(0x1234567u, 0x89abcdefu, (uint64_t)(j / 1000), (uint32_t)(j % 1000), lower, x)) return 3;
    fwrite(&x, 8, 1, stdout);
  }
}
""", "tn")
    m = 40_000
    for lower in (-40.0, -8.0, -2.0, -0.5, 0.0, 0.3, 2.0, 8.0, 40.0):
        out = subprocess.run([exe, repr(lower), str(m)], stdout=subprocess.PIPE, check=True).stdout
        x = np.frombuffer(out, dtype=np.float64)
        assert x.shape == (m,) and np.all(np.isfinite(x)) and np.all(x >= lower), lower
        u = np.exp(stats.norm.logsf(x) - stats.norm.logsf(lower))
        p = stats.kstest(u, "uniform").pvalue
        assert p > 1e-3, (lower, p)


# ---- resource guard ------------------------------------------------------------------------------------------------------------------------------

def test_parallel_latent_kernel_resources():
    """k_latents_par: no spilled VGPRs, no scratch (compile only, the product's flags)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not found")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    cxx = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).split()
    cmd = [hipcc, "--offload-arch=gfx950", *cxx, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, "dev_hip.hip"]
    out = subprocess.run(cmd, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert out.returncode == 0, out.stdout[-2000:]
    blocks = re.split(r"remark: Function Name: ", out.stdout)[1:]
    hit = [b for b in blocks if "13k_latents_parE" in b.split()[0]]       # (mangled name of s4b::k_latents_par)
    assert len(hit) == 1, [b.split()[0] for b in blocks]

    def field(name):
        return int(re.search(name + r": (\d+)", hit[0]).group(1))
    assert field("VGPRs Spill") == 0, hit[0]
    assert field(r"ScratchSize \[bytes/lane\]") == 0, hit[0]
    assert field(r"LDS Size \[bytes/block\]") == 0, hit[0]
