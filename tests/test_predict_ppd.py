"""s4b_predict_ppd without a GPU: the model of tests/ppd_cases.py against a brute-force loop over the emulated layer's predict_bart, philox_normal
compiled for the host against the numpy model, its tag against the counters of the latents, the moments of the model's deviates,
Stan4bartFit.predict_ppd over stand-in samplers, and the entry on the emulated device layer (no such kernels there: refused with its message).
The kernels are tested in tests/test_gpu_predict_ppd.py."""
import math
import os
import subprocess

import numpy as np
import pytest

import latent_par_cases as lp
import pd_cases as pc
import ppd_cases as pp
import summary_cases as sc
from conftest import friedman_case

LD = np.longdouble


@pytest.fixture(scope="module")
def emul_chain(emul_lib):
    args, _ = friedman_case(n=100, T=5, warmup=3, iter=6, ranef=False)
    args.keep_trees = True
    c = pc.Chain(emul_lib, "emu_", args, steps=(1, 2), rows=60)
    yield c
    c.close()


def test_model_against_a_brute_force_loop(emul_chain):
    rows, pool, key, first = 9, (3, 1), 0x9E3779B97F4A7C15, 5
    g = np.random.default_rng(2)
    x = emul_chain.x[:rows]
    off, dense = g.normal(size=rows), g.normal(size=(rows, 1))
    parts = [dict(bart=emul_chain.stored[S].predict_bart(x), sigma=g.uniform(0.5, 2.0, S), dense_coef=g.normal(size=(S, 1))) for S in pool]
    rs = g.uniform(0.5, 1.5, rows)
    probs = (0.0, 0.1, 0.5, 1.0)
    bart = np.concatenate([p["bart"] for p in parts], axis=1)
    y = bart.mean(axis=1) + off + g.normal(size=rows)
    ref, bd = pp.model(parts, key, probs, y=y, row_scale=rs, first_row=first, offset=off, dense=dense)
    S = sum(pool)
    sigma = np.concatenate([p["sigma"] for p in parts])
    coef = np.concatenate([p["dense_coef"] for p in parts])
    yrep, l, pv = np.zeros((rows, S)), np.zeros((rows, S)), np.zeros((rows, S))
    for i in range(rows):
        for k in range(S):
            z = bart[i, k] + off[i] + dense[i, 0] * coef[k, 0]
            w = [int(v) for v in lp.philox4x32_10(first + i, 0, k, 0x50504431, key & 0xFFFFFFFF, key >> 32)]
            u1 = (((w[0] << 21) ^ (w[1] >> 11)) + 0.5) * 2.0 ** -53
            u2 = (((w[2] << 21) ^ (w[3] >> 11)) + 0.5) * 2.0 ** -53
            sd = sigma[k] * rs[i]
            yrep[i, k] = z + sd * math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)
            r = (y[i] - z) / sd
            l[i, k] = -0.5 * math.log(2.0 * math.pi) - math.log(sd) - 0.5 * r * r
            pv[i, k] = 0.5 * math.erfc(-r / math.sqrt(2.0))
    np.testing.assert_allclose(ref["y_rep"], yrep, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(ref["quantiles"], np.quantile(yrep, probs, axis=1), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref["lpd"], np.log(np.exp(l).mean(axis=1)), rtol=1e-12)
    np.testing.assert_allclose(ref["lmean"], l.mean(axis=1), rtol=1e-12)
    np.testing.assert_allclose(ref["lm2"], l.var(axis=1) * S, rtol=1e-10)
    np.testing.assert_allclose(ref["pit"], pv.mean(axis=1), rtol=1e-12)
    for key_ in ("quantiles", "lpd", "lmean", "lm2", "pit"):
        assert bd[key_].shape == ref[key_].shape and np.all(bd[key_] > 0) and np.all(bd[key_] < 1e-9), key_
    # link 1: log Phi at the signed argument, both ends of |z|
    zb = np.linspace(-8.0, 8.0, rows * S).reshape(rows, S)
    yb = (np.arange(rows) % 2).astype(np.float64)
    r1, b1 = pp.score(zb, np.zeros_like(zb), yb, None, 1)
    want = np.array([[math.log(0.5 * math.erfc(-(t if yy else -t) / math.sqrt(2.0))) for t in row] for row, yy in zip(zb, yb)])
    np.testing.assert_allclose(r1["l"], want, rtol=1e-14)
    assert "pit" not in r1 and np.all(b1["lpd"] < 1e-12) and r1["l"].min() < -34.0
    with pytest.raises(AssertionError, match="link 1"):
        pp.score(zb * 1.01, np.zeros_like(zb), yb, None, 1)
    # one draw: lm2 = 0 and lpd = l
    r0, _ = pp.score(zb[:, :1], np.zeros((rows, 1)), zb[:, 0] + 1.0, np.full((rows, 1), 0.7), 0)
    assert np.array_equal(r0["lm2"], np.zeros(rows)) and np.array_equal(r0["lpd"], r0["l"][:, 0])


def test_tree_depth_follows_the_kernel_s_geometry():
    src = open(os.path.join(lp.CSRC, "dev_ppd.inc")).read()
    assert "const int W = R >= 4 ? 1 : 4 / R, slots = 4 / W;" in src and "for (int64_t k = sub * 64 + lane; k < S; k += 64 * W)" in src
    assert [pp.tree_depth(S) for S in (1, 64, 65, 1024, 1025, 2048, 2049, 4108, 16380)] == [7, 7, 8, 22, 16, 23, 18, 26, 73]


PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "philox.hpp"
int main() {
  unsigned long long key, row; unsigned draw;
  while (std::scanf("%llx %llu %u", &key, &row, &draw) == 3) {
    const double e = s4b::philox_normal((uint32_t)key, (uint32_t)(key >> 32), (uint64_t)row, (uint32_t)draw);
    uint64_t b; std::memcpy(&b, &e, 8);
    std::printf("%016" PRIx64 "\n", b);
  }
  return 0;
}
"""


def test_philox_normal_on_the_host_against_the_model(tmp_path):
    g = np.random.default_rng(3)
    keys = [0x0123456789ABCDEF, 0x00000000DEADBEEF, 0xC2B2AE3D00000000, (1 << 64) - 1, 0]          # a zero low half, a zero high half, all ones, all zeros
    triples = [(k, r, d) for k in keys for r in (0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 7, (1 << 63) + 5) for d in (0, 1, 63, 64, 16383)]
    triples += [(int(g.integers(0, 1 << 63)) * 2 + 1, int(g.integers(0, 1 << 40)), int(g.integers(0, 16384))) for _ in range(200)]
    src, exe = tmp_path / "phx.cpp", tmp_path / "phx"
    src.write_text(PROGRAM)
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-I", lp.CSRC, "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], input="".join(f"{k:x} {r} {d}\n" for k, r, d in triples), stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    assert len(out) == len(triples) >= 300
    got = np.array([int(w, 16) for w in out], dtype=np.uint64).view(np.float64)
    worst = 0.0
    for (k, r, d), e_host in zip(triples, got):
        e, be = pp.noise(k, [r], [d], lp.GLIBC)
        worst = max(worst, abs(float(LD(e_host) - e[0, 0])) / float(be[0, 0]))
    print(f"philox_normal on the host, {len(triples)} triples: max |host - model| / bound = {worst:.3g}")
    assert worst <= pp.BOUND_FACTOR
    assert any(r >= 1 << 32 for _, r, _ in triples) and any(d == 16383 for _, _, d in triples)
    # the row's high word and the draw reach the counter: other deviates
    base = pp.noise(keys[0], [5], [7])[0][0, 0]
    assert pp.noise(keys[0], [5 + (1 << 32)], [7])[0][0, 0] != base and pp.noise(keys[0], [5], [8])[0][0, 0] != base and pp.noise(keys[1], [5], [7])[0][0, 0] != base


def test_tag_differs_from_every_counter_of_the_latents():
    """philox_trunc_normal's counters are {draw low, draw high, observation, attempt} with attempt < TN_MAX_ATTEMPTS; philox_normal's last word is the
    tag: beyond every attempt number, so that no block is shared under one key whatever the other three words."""
    tag, attempts = pp.header_constants()
    lp.kernel_geometry()          # (asserts the latents' counter layout and that the attempt is the last word)
    assert tag == pp.PPD_TAG == 0x50504431 and attempts == lp.MAX_ATTEMPTS and tag >= attempts
    a = lp.philox4x32_10(3, 0, 9, tag, 11, 22)
    for t in (0, 1, attempts - 1):
        b = lp.philox4x32_10(3, 0, 9, t, 11, 22)
        assert [int(v) for v in a] != [int(v) for v in b]


def test_model_deviates_have_mean_0_and_variance_1():
    e, be = pp.noise(0x243F6A8885A308D3, np.arange(1000), np.arange(100))
    x = e.astype(np.float64).ravel()
    n = x.size
    assert n == 100000 and np.all(np.isfinite(x)) and be.max() < 1e-14
    assert abs(x.mean()) <= 5.0 / math.sqrt(n), x.mean()
    assert abs(x.var() - 1.0) <= 5.0 * math.sqrt(2.0 / n), x.var()


def test_entry_is_refused_on_the_emulated_layer(emul_lib, emul_chain):
    assert hasattr(emul_lib, "emu_predict_ppd")
    x = emul_chain.x[:7]
    for smp, S in ((emul_chain.live, 3), (emul_chain.stored[3], 3)):
        before = emul_chain.live.get_counters()
        with pytest.raises(RuntimeError, match="no posterior predictive kernels"):
            smp.predict_ppd(x, [0.025, 0.975], sigma=np.ones(S))
        with pytest.raises(RuntimeError, match="no posterior predictive kernels"):
            smp.predict_ppd(x, y=np.zeros(7), sigma=np.ones(S), peers=[emul_chain.stored[1]], peer_sigma=[np.ones(1)])
        assert not any(smp.ppd_info.values()) and np.array_equal(emul_chain.live.get_counters(), before)
        with pytest.raises(ValueError, match="probs must be a vector"):
            smp.predict_ppd(x, [[0.5, 0.6]], sigma=np.ones(S))
        with pytest.raises(ValueError, match=r"sigma must have shape \(3,\)"):
            smp.predict_ppd(x, [0.5], sigma=np.ones(4))
        with pytest.raises(ValueError, match=r"peer_sigma\[0\] must be \[1 x 1\]"):
            smp.predict_ppd(x, [0.5], sigma=np.ones(S), peers=[emul_chain.stored[1]], peer_sigma=[np.ones(3)])


def test_oracle_library_has_no_entry(oracle_lib):
    from stan4bart_amd.abi import Sampler
    s = Sampler.__new__(Sampler)
    s._lib, s._pfx = oracle_lib, "orc_"
    with pytest.raises(RuntimeError, match="no predict_ppd"):
        Sampler.predict_ppd(s, np.zeros((2, 3)), [0.5])


class _Recorder:
    """A stand-in sampler: records the call and answers with fixed scores and the probs (plus the row number) as quantiles."""

    def __init__(self, draws=15):
        self.calls, self.draws = [], draws

    def predict_ppd(self, x, probs, **kw):
        self.calls.append(dict(x=x, probs=np.array(probs), **kw))
        n = len(x)
        scored = kw.get("y") is not None
        return dict(quantiles=np.asarray(probs)[:, None] * 10.0 + np.arange(n)[None, :], lpd=-1.0 - 0.01 * np.arange(n) if scored else None,
                    lmean=None, lm2=0.5 + 0.1 * np.arange(n) if scored else None, pit=np.full(n, 0.25) if scored and not kw.get("link") else None,
                    draws=self.draws, info={})


class _NoSampler:
    def predict_ppd(self, *a, **k):
        raise AssertionError("the ABI was called although the arguments had to be refused")


def test_fit_hands_sigma_per_chain_row_scale_and_the_key_down():
    a, b, c = _Recorder(), _NoSampler(), _NoSampler()          # the first sampler takes the call, the others travel as its peers
    fit, new_terms, q = sc.fake_fit(0, n_chain=3, samplers=[a, b, c])
    g = np.random.default_rng(4)
    x, X, off, w = g.normal(size=(40, 3)), g.normal(size=(40, 2)), g.normal(size=40), g.uniform(0.5, 4.0, 40)
    out = fit.predict_ppd(x, X=X, groups=new_terms, offset=off, obs_weights=w, seed=5)
    assert np.array_equal(out["probs"], (0.025, 0.5, 0.975)) and out["quantiles"].shape == (3, 40) and out["draws"] == 15 and len(a.calls) == 1
    assert not {"lpd", "pit", "coverage", "elpd_waic"} & set(out)
    call = a.calls[0]
    sig = fit.stan[fit.par_names.index("aux.1")]
    assert np.array_equal(call["sigma"], sig[:, 0]) and len(call["peer_sigma"]) == 2
    assert np.array_equal(call["peer_sigma"][0], sig[:, 1]) and np.array_equal(call["peer_sigma"][1], sig[:, 2]) and not np.array_equal(sig[:, 1], sig[:, 2])
    assert np.array_equal(call["row_scale"], 1.0 / np.sqrt(w)) and call["y"] is None and call["link"] == 0 and call["peers"] == [b, c]
    linear = fit._summary_linear("ev", X, new_terms, off, True, np.random.default_rng(5))          # the same seed: predict's draws of unseen levels
    want = [linear(ch) for ch in range(3)]
    assert want[0]["ell_index"].max() >= q, "no unseen level reached the table"
    for key in ("offset", "dense", "dense_coef", "ell_index", "ell_value", "ell_coef"):
        assert np.array_equal(call[key], want[0][key]), key
    for ch in (1, 2):
        assert np.array_equal(call["peer_dense_coef"][ch - 1], want[ch]["dense_coef"]) and np.array_equal(call["peer_ell_coef"][ch - 1], want[ch]["ell_coef"])
    # the key: a function of the seed, returned, and the returned seed repeats a call made without one
    assert out["noise_key"] == call["noise_key"] and 0 <= out["noise_key"] < 1 << 64 and out["seed"] == 5
    again = fit.predict_ppd(x, seed=5)
    assert again["noise_key"] == out["noise_key"] and a.calls[-1]["row_scale"] is None
    assert fit.predict_ppd(x, seed=6)["noise_key"] != out["noise_key"]
    f1, f2 = fit.predict_ppd(x, groups=new_terms), fit.predict_ppd(x, groups=new_terms)
    assert f1["noise_key"] != f2["noise_key"]
    rep = fit.predict_ppd(x, groups=new_terms, seed=f1["seed"])
    assert rep["noise_key"] == f1["noise_key"] and np.array_equal(a.calls[-1]["ell_coef"], a.calls[-3]["ell_coef"])


def test_fit_derives_waic_se_and_coverage_on_the_host():
    a = _Recorder(draws=15)
    fit, _, _ = sc.fake_fit(1, n_chain=1, samplers=[a])
    n = 12
    x = np.zeros((n, 3))
    y = np.arange(n) + np.where(np.arange(n) % 3 == 0, 20.0, 5.0)          # quantiles are row + 10 p: a third of the rows lies outside [row + 1, row + 9]
    out = fit.predict_ppd(x, y=y, probs=(0.5, 0.9, 0.1), seed=1)
    assert np.array_equal(a.calls[0]["y"], y) and a.calls[0]["peers"] == [] and a.calls[0]["peer_sigma"] == []
    lpd, lm2 = -1.0 - 0.01 * np.arange(n), 0.5 + 0.1 * np.arange(n)
    assert np.array_equal(out["lpd"], lpd) and np.array_equal(out["p_waic"], lm2 / 14) and np.array_equal(out["elpd_waic"], lpd - lm2 / 14)
    assert out["elpd_waic_total"] == float((lpd - lm2 / 14).sum())
    assert out["se"] == pytest.approx(math.sqrt(n * np.var(lpd - lm2 / 14, ddof=1)), rel=1e-14)
    assert np.array_equal(out["pit"], np.full(n, 0.25))
    assert out["coverage"] == pytest.approx(8 / 12)          # the outermost pair is (0.1, 0.9), whatever the order of probs
    one = fit.predict_ppd(x, y=y, probs=(0.5,), seed=1)
    assert "coverage" not in one and "lpd" in one
    none = fit.predict_ppd(x, y=y, probs=(), seed=1)
    assert none["quantiles"].shape == (0, n) and "coverage" not in none


def test_python_refusals():
    fit, _, _ = sc.fake_fit(0, samplers=[_NoSampler(), _NoSampler()])
    x = np.zeros((40, 3))
    with pytest.raises(ValueError, match="predict_ppd needs x_bart"):
        fit.predict_ppd()
    for bad in ((-0.1, 0.5), (0.5, 1.5), (np.nan,), ((0.1, 0.2),), np.linspace(0, 1, 17)):
        with pytest.raises(ValueError, match=r"'probs' must be a vector of at most 16 values in \[0, 1\]"):
            fit.predict_ppd(x, probs=bad)
    with pytest.raises(ValueError, match="nothing asked for"):
        fit.predict_ppd(x, probs=())
    with pytest.raises(ValueError, match=r"y must have shape \[40\]"):
        fit.predict_ppd(x, y=np.zeros(39))
    for bad in (np.zeros(40), np.full(40, np.inf), np.ones(39), -np.ones(40)):
        with pytest.raises(ValueError, match="obs_weights must be 40 finite values > 0"):
            fit.predict_ppd(x, obs_weights=bad)
    bare, _, _ = sc.fake_fit(0)
    with pytest.raises(ValueError, match="predict_ppd requires 'bart_args' to contain 'keepTrees'"):
        bare.predict_ppd(x)
    # a binary response: no replicate, so no quantile; the scores go through with link 1, no sigma and no pit
    binary, _, _ = sc.fake_fit(0, family="binomial", samplers=[_NoSampler()])
    with pytest.raises(ValueError, match="Bernoulli\\(mean of ev\\), which predict_summary gives"):
        binary.predict_ppd(x)
    rec = _Recorder()
    scored, _, _ = sc.fake_fit(0, family="binomial", n_chain=1, samplers=[rec])
    out = scored.predict_ppd(x, y=np.zeros(40), probs=())
    assert rec.calls[0]["link"] == 1 and rec.calls[0]["sigma"] is None and rec.calls[0]["peer_sigma"] is None and "pit" not in out and "lpd" in out
    # the siblings still refuse 'ppd' with their message
    for name in ("predict_summary", "partial_dependence", "predict_quantiles", "predict_contrast"):
        with pytest.raises(ValueError, match=f"{name} does not form 'ppd': its noise is drawn per element of the draws matrix \\(use predict\\)"):
            getattr(fit, name)(*((0,) if name == "partial_dependence" else ()), x_bart=x, type="ppd")
