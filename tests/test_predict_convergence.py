"""s4b_predict_convergence without a GPU: the model of tests/conv_cases.py against parallel.split_rhat, against an FFT evaluation of the autocovariance,
against the known effective sample size of AR(1) series and against cases worked by hand; the share of rows the bound leaves out at every pool shape
of the GPU tests; Stan4bartFit.predict_convergence over stand-in samplers, every Python-side refusal, the entry on the emulated device layer (no such
kernel there: refused with its message) and the geometry constants the model depends on.  The kernel is tested in
tests/test_gpu_predict_convergence.py."""
import math
import os

import numpy as np
import pytest

import conv_cases as cc
import latent_par_cases as lp
import pd_cases as pc
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


def _one(x, lens, split=False):
    starts, N = cc.chains(lens, split)
    r = cc.estimate(np.asarray(x, dtype=np.float64)[None, :], starts, N)
    return {k: (int(r[k][0]) if k == "n_pairs" else float(r[k][0])) for k in ("rhat", "ess", "tau", "n_pairs", "mean", "mcse")}


def test_chains_are_cut_from_the_back_and_split_around_the_middle_draw():
    assert cc.chains((13, 5), False) == ([0, 13], 5)
    assert cc.chains((13, 5), True) == ([0, 3, 13, 16], 2)
    assert cc.chains((9,), True) == ([0, 5], 4)          # draws 0 .. 3 and 5 .. 8: draw 4 belongs to neither half
    assert cc.chains((8, 9), True) == ([0, 4, 8, 12], 4)          # the longer chain loses its last draw first, then has no middle draw
    assert cc.chains((13, 9, 13), True) == ([0, 5, 13, 18, 22, 27], 4)
    assert [cc.j_limit(n) for n in (4, 5, 6, 7, 8, 9, 66, 67, 68, 130, 132)] == [0, 0, 1, 1, 2, 2, 31, 31, 32, 63, 64]
    core = open(os.path.join(lp.CSRC, "sampler_core.hpp")).read()
    assert "if (split) start.push_back((int32_t)(at + n0 - h));" in core and "return (int)(split ? h : n0);" in core
    assert "if (numChains > 256) throw" in core


def test_rhat_of_the_model_is_split_rhat():
    from stan4bart_amd.parallel import split_rhat
    g = np.random.default_rng(2)
    for chains_, samples in ((2, 40), (4, 10), (3, 8)):
        draws = g.normal(size=(chains_, 25, samples)) + 0.4 * g.normal(size=(chains_, 25, 1))
        x = np.concatenate([draws[c] for c in range(chains_)], axis=1)          # [pars x pooled draws]
        starts, N = cc.chains((samples,) * chains_, True)
        got = cc.estimate(x, starts, N)["rhat"].astype(np.float64)
        np.testing.assert_allclose(got, split_rhat(draws), rtol=1e-13)
        assert got.max() > 1.05
    one = cc.estimate(g.normal(size=(3, 12)), *cc.chains((12,), False))
    assert np.all(np.isnan(one["rhat"])) and np.all(np.isfinite(one["ess"]))          # one chain unsplit: no rhat, but an ess


def test_autocovariance_of_the_model_against_an_fft_evaluation():
    """numpy's FFT gives the lag sums s(t) = sum_{i < N - t} d[i] d[i + t]; the unbiased estimate divides them by N - t.  The model divides by N at
    every lag — the estimator of the autocovariance header that Stan's effective-sample-size header calls (DESIGN.md 5.11 records that the issue's
    text said N - t and that the header decides) — so N a(t) = (N - t) a_fft(t) = s(t)."""
    g = np.random.default_rng(3)
    for N in (7, 64, 130, 1000):
        x = cc.ar1(0.8, N, g, (4, 2))          # [rows x chains x N]
        d = (x - x.mean(axis=2, keepdims=True)).astype(LD)
        f = np.fft.rfft(d.astype(np.float64), 2 * N, axis=2)
        s = np.fft.irfft(f * np.conj(f), 2 * N, axis=2)[:, :, :N]
        scale = (d * d).sum(axis=2).astype(np.float64)
        for t in (0, 1, 2, 3, N // 2, N - 3, N - 1):
            a_fft = s[:, :, t] / (N - t)
            a = cc.acov(d, t).astype(np.float64)
            assert np.all(np.abs(a * N - a_fft * (N - t)) <= 1e-12 * scale), (N, t)
        assert np.array_equal(cc.acov(d, 0), (d * d).sum(axis=2) / LD(N))


@pytest.mark.parametrize("phi", [0.0, 0.5, 0.9])
def test_ar1_series_have_their_known_effective_sample_size(phi):
    """AR(1) with coefficient phi has integrated autocorrelation time (1 + phi) / (1 - phi): ess = D (1 - phi) / (1 + phi).  4 chains of 2 000 draws,
    48 rows, seed fixed.  The margin: the truncated estimator sums about 2 M autocorrelations of variance about 1 / D each, M = the lag the sequence
    stops at (a few times the autocorrelation time, under 100 lags at phi = 0.9), so one row's tau has a relative sd of at most sqrt(2 * 200 / 8000) =
    0.22 and the mean over 48 rows 0.032; Geyer's truncation adds a bias of a few percent.  Allowed: 12 % for the mean over the rows (three sd and
    the bias), 100 % for a single row (four sd)."""
    g = np.random.default_rng([77, int(phi * 10)])
    rows, C, N = 48, 4, 2000
    x = cc.ar1(phi, N, g, (rows, C)).reshape(rows, C * N)
    starts, n = cc.chains((N,) * C, False)
    r = cc.estimate(x, starts, n)
    want = C * N * (1.0 - phi) / (1.0 + phi)
    ess = r["ess"].astype(np.float64)
    print(f"AR(1) phi {phi}: ess {ess.min():.0f} .. {ess.max():.0f}, mean {ess.mean():.0f}, theory {want:.0f}; n_pairs {r['n_pairs'].min()} .. {r['n_pairs'].max()}")
    assert abs(ess.mean() / want - 1.0) <= 0.12 and np.all(np.abs(ess / want - 1.0) <= 1.0)
    assert np.all(np.abs(r["rhat"].astype(np.float64) - 1.0) < 0.05)
    split = cc.estimate(x, *cc.chains((N,) * C, True))["ess"].astype(np.float64)
    assert abs(split.mean() / want - 1.0) <= 0.12
    # mcse is the pooled sd over sqrt(ess)
    sd = x.std(axis=1, ddof=1)
    np.testing.assert_allclose(r["mcse"].astype(np.float64), sd / np.sqrt(ess), rtol=1e-12)
    np.testing.assert_allclose(r["mean"].astype(np.float64), x.mean(axis=1), rtol=0, atol=1e-13)


def test_cases_worked_by_hand():
    """One chain: rho(t) = A(t) / q - 1 / (N - 1) with A(t) the lag sum and q = A(0) (W = q / (N - 1), var+ = q / N, divisor N).
      N = 4, 5   the limit is pair 0: J = 0, tau = -1 + 2 * 1 + 1 = 2 whatever the data, ess = D / 2.
      N = 6      x = 1 .. 6: d = -2.5 .. 2.5, q = 17.5, A(1) = 8.75, A(2) = 1, A(3) = -4.75: rho = 1, 0.3, -1/7, -33/70.  P_0 = 1.3 > 0, pair 1 is the
                 limit: J = 1, P_1 < 0 so it is zeroed, e_1 < 0 so no tail term: tau = -1 + 2 * 1.3 = 1.6, ess = 3.75.
      N = 7      x = 1 -1 1 -2 1 -1 1: mean 0, q = 10, A(1) = -8, A(2) = 7, A(3) = -6: rho(1) = -29/30, P_0 = 1/30 > 0; J = 1; rho(2) = 8/15,
                 rho(3) = -23/30, P_1 = -7/30 < 0: zeroed, but e_1 = 8/15 > 0 is the tail term: tau = -1 + 2 / 30 + 8 / 15 = -0.4, ess = -17.5
                 (Stan returns the negative value too).
    Two chains:
      N = 6      1 .. 6 and the same shifted by sqrt(7 / 6): B' = 7 / 12 = W / 6, so var+ = W = 3.5, rhat = 1, rho(t) = A(t) / 21: P_0 = 29.75 / 21,
                 J = 1, P_1 = -3.75 / 21 zeroed, e_1 = 1 / 21 > 0: tau = -1 + 59.5 / 21 + 1 / 21 = 39.5 / 21, ess = 12 * 21 / 39.5.
      N = 7      the N = 7 series twice: B' = 0, rho as for one chain, tau = -0.4, ess = -35, rhat = sqrt(6 / 7)."""
    for lens, D in (((4,), 4), ((5,), 5), ((4, 4), 8), ((5, 5), 10)):
        r = _one(np.random.default_rng(D).normal(size=sum(lens)), lens)
        assert r["n_pairs"] == 0 and r["tau"] == 2.0 and r["ess"] == D / 2.0, (lens, r)
    r = _one([1, 2, 3, 4, 5, 6], (6,))
    assert r["n_pairs"] == 1 and r["tau"] == pytest.approx(1.6, rel=1e-15) and r["ess"] == pytest.approx(3.75, rel=1e-15) and math.isnan(r["rhat"])
    assert r["mean"] == 3.5 and r["mcse"] == pytest.approx(math.sqrt(3.5 / 3.75), rel=1e-15)
    seven = [1, -1, 1, -2, 1, -1, 1]
    r = _one(seven, (7,))
    assert r["n_pairs"] == 1 and r["tau"] == pytest.approx(-0.4, rel=1e-14) and r["ess"] == pytest.approx(-17.5, rel=1e-14) and math.isnan(r["mcse"])
    r = _one([1, 2, 3, 4, 5, 6] + [v + math.sqrt(7.0 / 6.0) for v in range(1, 7)], (6, 6))
    assert r["n_pairs"] == 1 and r["tau"] == pytest.approx(39.5 / 21.0, rel=1e-14) and r["ess"] == pytest.approx(12.0 * 21.0 / 39.5, rel=1e-14)
    assert r["rhat"] == pytest.approx(1.0, rel=1e-14)
    r = _one(seven + seven, (7, 7))
    assert r["n_pairs"] == 1 and r["tau"] == pytest.approx(-0.4, rel=1e-14) and r["ess"] == pytest.approx(-35.0, rel=1e-14)
    assert r["rhat"] == pytest.approx(math.sqrt(6.0 / 7.0), rel=1e-15)
    # the same series as the two halves of ONE chain of 13 and of 14 draws: the middle draw of the odd length plays no part
    assert _one(seven[:6] + [99.0] + seven[:6], (13,), True) == _one(seven[:6] + seven[:6], (12,), True)
    a, b = _one(seven + seven, (14,), True), _one(seven + seven, (7, 7))
    assert all(a[k] == b[k] for k in ("rhat", "ess", "tau", "n_pairs", "mean")) and math.isnan(a["mcse"])          # (the root of a negative ess)


def test_monotone_pass_and_the_last_pair():
    """A sequence built backwards from chosen pair sums: three chains far apart (var+ >> W: every rho near 1) make every P_j > 0, so J is the limit
    and P'_j the running minimum; the sum is then checked against one formed from the model's own rho(t) pair by pair in plain Python."""
    g = np.random.default_rng(9)
    N, C = 20, 3
    x = (cc.ar1(0.3, N, g, (5, C)) + 6.0 * np.arange(C)[None, :, None]).reshape(5, C * N)
    starts, n = cc.chains((N,) * C, False)
    r = cc.estimate(x, starts, n)
    assert cc.j_limit(N) == 8 and np.all(r["n_pairs"] == 8)
    X = x.reshape(5, C, N).astype(LD)
    d = X - X.mean(axis=2, keepdims=True)
    W = ((d * d).sum(axis=2) / (N - 1)).mean(axis=1)
    vp = W * (N - 1) / N + X.mean(axis=2).var(axis=1, ddof=1)
    for i in range(5):
        rho = [1.0] + [float(1 - (W[i] - cc.acov(d[i:i + 1], t)[0].mean()) / vp[i]) for t in range(1, 18)]
        P = [rho[2 * j] + rho[2 * j + 1] for j in range(9)]
        assert all(p > 0 for p in P)
        run, total = math.inf, 0.0
        for j in range(8):
            run = min(run, P[j])
            total += run
        tau = -1.0 + 2.0 * (total + rho[16]) + rho[16]          # pair 8 is kept as it is (its sum is >= 0), its even entry is also the tail term
        assert float(r["tau"][i]) == pytest.approx(tau, rel=1e-12)
    assert sorted(P, reverse=True) != P, "the pair sums are monotone already: the case tests no running minimum"


def test_rows_without_an_answer():
    g = np.random.default_rng(1)
    starts, N = cc.chains((8, 8), False)
    x = g.normal(size=(6, 16))
    x[1, 3] = np.nan
    x[2, 9] = np.inf
    x[3] = 0.7                      # every chain constant
    x[4, :8] = 0.1                  # one chain constant, the other not: an answer (0.1 * 8 / 8 != 0.1 in floating point: the exact rule matters)
    r = cc.estimate(x, starts, N)
    assert list(r["answer"]) == [True, False, False, False, True, True] and list(r["n_pairs"][1:4]) == [-1, -1, -1]
    for key in cc.OUTPUTS:
        assert np.all(np.isnan(r[key][1:4])) and np.all(np.isfinite(r[key][[0, 4, 5]]))
    short = cc.estimate(x, *cc.chains((3, 3), False))
    assert not short["answer"].any()
    # a value that is not finite OUTSIDE the draws used (the middle draw, the cut tail) does not matter
    y = g.normal(size=(2, 22))
    y[0, 4], y[0, 10], y[1, 17], y[1, 12] = np.nan, np.inf, np.nan, -np.inf
    r = cc.estimate(y, *cc.chains((13, 9), True))          # N0 = 9: halves of 4; draw 4 of each chain (4 and 17) and draws 9 .. 12 of the first unused
    assert cc.chains((13, 9), True) == ([0, 5, 13, 18], 4) and np.all(r["answer"])


@pytest.mark.parametrize("name", list(cc.POOLS))
def test_share_left_out_at_the_pool_shapes_of_the_gpu_tests(name):
    """The model alone, on series of the GPU cases' kind with the input error of a value kernel with two dense columns: the perturbed runs agree on J
    in all but 2 % of the rows (from_x asserts it) and the tolerance stays of the order of the rounding error times the conditioning."""
    lens, split = cc.POOLS[name]
    rows = 200 if sum(lens) <= 2300 else 12
    x = cc.synthetic(lens, rows, 3)
    starts, N = cc.chains(lens, split)
    ref, bd, compared = cc.from_x(x, 5.0 * cc.U * (1.0 + np.abs(x)), starts, N, what=name)
    left = int((ref["answer"] & ~compared).sum())
    assert left <= 0.02 * rows
    if N < 4:
        assert not ref["answer"].any()
        return
    assert ref["answer"].all() and np.all(ref["n_pairs"] <= cc.j_limit(N))
    with np.errstate(invalid="ignore"):          # (mcse is NaN where ess < 0: short chains)
        rel = {k: float(np.nanmax(bd[k][compared] / np.maximum(np.abs(ref[k][compared]), 1e-300))) for k in cc.OUTPUTS if not (k == "rhat" and len(starts) == 1)}
    assert np.array_equal(np.isnan(ref["mcse"]), ref["ess"] < 0)
    print(f"pool {name}: {len(starts)} chains of {N}, n_pairs {ref['n_pairs'].min()} .. {ref['n_pairs'].max()}, {left} row(s) left out, largest relative bound "
          + ", ".join(f"{k} {v:.3g}" for k, v in rel.items()))
    assert all(0 < v < 1e-8 for k, v in rel.items() if k != "mean"), rel


def test_likelihood_series_is_scaled_by_the_row_maximum():
    l = np.array([[-3.0, -1.0, -900.0, -2.0], [-800.0, -800.5, -801.0, -799.0]])
    x, bx = cc.lik_series(l, 1e-15)
    assert np.array_equal(x[0], np.exp(l[0] + 1.0)) and x[0, 2] == 0.0 and x[0, 1] == 1.0 and x[1, 3] == 1.0
    assert np.all(bx >= 0) and bx[0, 2] == 0.0
    a = cc.estimate(np.exp(l[1:] + 799.0), [0], 4)
    b = cc.estimate(7.0 * np.exp(l[1:] + 799.0), [0], 4)
    assert float(a["ess"][0]) == float(b["ess"][0]) and float(b["mean"][0]) == pytest.approx(7.0 * float(a["mean"][0]), rel=1e-15)


def test_geometry_the_model_depends_on():
    src = open(os.path.join(lp.CSRC, "dev_conv.inc")).read()
    assert "constexpr int CV_LAGS = 64;" in src and "constexpr int CV_RED = 16;" in src and "constexpr int CV_CHAINS_MAX = 256;" in src
    assert "const int W = R >= 4 ? 1 : 4 / R, slots = 4 / W;" in src
    assert "for (int k = lane; k < N; k += 64)" in src and "for (int c = lane; c < C; c += 64)" in src          # (Ll, Lc of the bound)
    assert "for (; k + 3 < n; k += 4)" in src and "for (int c = m; c < C; c += 4)" in src and "g += (p0 + p1) + (p2 + p3);" in src
    assert "const double mu = lo == hi ? lo : s / dN;" in src          # (the exact rule for a constant chain)
    assert "const int jmax = N >= 4 ? (N - 4) / 2 : 0;" in src
    assert "(size_t)8 * CV_RED + (size_t)16 * (size_t)slots * (size_t)c.numChains" in src and "(size_t)8 * (size_t)slots * 4 * CV_LAGS" in src
    assert "atomic" not in src.split("struct ConvDev")[1]
    assert cc.lds_bytes(16384, 256) == 131072 + 128 + 4096 + 2048 <= 160 * 1024 and cc.lds_bytes(1024, 256) == 32768 + 128 + 16384 + 8192
    hip = open(os.path.join(lp.CSRC, "dev_hip.hip")).read()
    assert '#include "dev_loo.inc"\n#include "dev_conv.inc"\n' in hip
    assert "dev_conv.inc" in open(os.path.join(lp.CSRC, "Makefile")).read()


def test_entry_is_refused_on_the_emulated_layer(emul_lib, emul_chain):
    assert hasattr(emul_lib, "emu_predict_convergence")
    x = emul_chain.x[:7]
    for smp, S in ((emul_chain.live, 3), (emul_chain.stored[3], 3)):
        before = emul_chain.live.get_counters()
        with pytest.raises(RuntimeError, match="no chain kernels"):
            smp.predict_convergence(x)
        with pytest.raises(RuntimeError, match="no chain kernels"):
            smp.predict_convergence(x, quantity="lik", y=np.zeros(7), sigma=np.ones(S), peers=[emul_chain.stored[1]], peer_sigma=[np.ones(1)])
        assert not any(smp.conv_info.values()) and np.array_equal(emul_chain.live.get_counters(), before)
        with pytest.raises(ValueError, match="outputs must name at least one of"):
            smp.predict_convergence(x, outputs=())
        with pytest.raises(ValueError, match="outputs must name at least one of"):
            smp.predict_convergence(x, outputs=("rhat", "khat"))
        with pytest.raises(ValueError, match="quantity must be one of"):
            smp.predict_convergence(x, quantity="ppd")
        with pytest.raises(ValueError, match=r"y must have shape \(7,\)"):
            smp.predict_convergence(x, quantity="lik", y=np.zeros(8), sigma=np.ones(S))
        with pytest.raises(ValueError, match=r"sigma must have shape \(3,\)"):
            smp.predict_convergence(x, quantity="lik", y=np.zeros(7), sigma=np.ones(4))
        with pytest.raises(ValueError, match=r"peer_sigma\[0\] must be \[1 x 1\]"):
            smp.predict_convergence(x, quantity="lik", y=np.zeros(7), sigma=np.ones(S), peers=[emul_chain.stored[1]], peer_sigma=[np.ones(3)])


def test_oracle_library_has_no_entry(oracle_lib):
    from stan4bart_amd.abi import Sampler
    s = Sampler.__new__(Sampler)
    s._lib, s._pfx = oracle_lib, "orc_"
    with pytest.raises(RuntimeError, match="no predict_convergence"):
        Sampler.predict_convergence(s, np.zeros((2, 3)))


class _Recorder:
    """A stand-in sampler: records the call and answers with fixed per-row results."""

    def __init__(self, chains=6, chain_len=2):
        self.calls, self.chains, self.chain_len = [], chains, chain_len

    def predict_convergence(self, x, **kw):
        self.calls.append(dict(x=x, **kw))
        n = len(x)
        rhat = 1.0 + 0.002 * np.arange(n)
        rhat[3] = np.nan
        ess = 10.0 + np.arange(n)
        ess[3] = np.nan
        return dict(rhat=rhat, ess=ess, mean=np.arange(n) * 0.5, mcse=np.full(n, 0.1), n_pairs=np.where(np.arange(n) == 3, -1, 2).astype(np.int32),
                    draws=15, chains=self.chains, chain_len=self.chain_len, info={})


class _NoSampler:
    def predict_convergence(self, *a, **k):
        raise AssertionError("the ABI was called although the arguments had to be refused")


def test_fit_pools_the_chains_in_one_call():
    a, b, c = _Recorder(), _NoSampler(), _NoSampler()          # the first sampler takes the call, the others travel as its peers
    fit, new_terms, q = sc.fake_fit(0, n_chain=3, samplers=[a, b, c])
    g = np.random.default_rng(4)
    x, X, off, w, y = g.normal(size=(40, 3)), g.normal(size=(40, 2)), g.normal(size=40), g.uniform(0.5, 4.0, 40), g.normal(size=40)
    out = fit.predict_convergence(x, X=X, groups=new_terms, offset=off, seed=5)
    call = a.calls[0]
    assert call["quantity"] == "ev" and call["split"] is True and call["y"] is None and call["sigma"] is None and call["peer_sigma"] is None
    assert call["row_scale"] is None and call["link"] == 0 and call["peers"] == [b, c]
    linear = fit._summary_linear("ev", X, new_terms, off, True, np.random.default_rng(5))          # the same seed: predict's draws of unseen levels
    want = [linear(ch) for ch in range(3)]
    assert want[0]["ell_index"].max() >= q, "no unseen level reached the table"
    for key in ("offset", "dense", "dense_coef", "ell_index", "ell_value", "ell_coef"):
        assert np.array_equal(call[key], want[0][key]), key
    for ch in (1, 2):
        assert np.array_equal(call["peer_dense_coef"][ch - 1], want[ch]["dense_coef"]) and np.array_equal(call["peer_ell_coef"][ch - 1], want[ch]["ell_coef"])
    # what the host derives: NaN rows count nowhere
    n = 40
    assert out["rhat_max"] == 1.0 + 0.002 * 39 and out["n_high_rhat"] == int(np.sum(1.0 + 0.002 * np.delete(np.arange(n), 3) > 1.01)) == 34
    assert out["ess_min"] == 10.0 and out["chains"] == 6 and out["chain_len"] == 2 and out["draws"] == 12 and "r_eff" not in out
    assert np.isnan(out["rhat"][3]) and out["n_pairs"][3] == -1 and np.array_equal(out["mean"], np.arange(n) * 0.5)
    assert fit.predict_convergence(x, rhat_threshold=1.05)["n_high_rhat"] == int(np.sum(1.0 + 0.002 * np.delete(np.arange(n), 3) > 1.05))
    # the likelihood: sigma per chain, the row scale of the observation weights, r_eff per row
    lik = fit.predict_convergence(x, X=X, groups=new_terms, offset=off, quantity="lik", y=y, obs_weights=w, split=False, seed=5)
    call = a.calls[-1]
    sig = fit.stan[fit.par_names.index("aux.1")]
    assert call["quantity"] == "lik" and call["split"] is False and np.array_equal(call["y"], y) and np.array_equal(call["row_scale"], 1.0 / np.sqrt(w))
    assert np.array_equal(call["sigma"], sig[:, 0]) and np.array_equal(call["peer_sigma"][0], sig[:, 1]) and np.array_equal(call["peer_sigma"][1], sig[:, 2])
    assert np.array_equal(np.delete(lik["r_eff"], 3), np.delete(lik["ess"], 3) / 12.0) and np.isnan(lik["r_eff"][3])
    # "indiv.bart": no linear part
    fit.predict_convergence(x, X=X, groups=new_terms, offset=off, type="indiv.bart")
    assert a.calls[-1]["dense"] is None and a.calls[-1]["ell_index"] is None and a.calls[-1]["offset"] is None
    # a binary response goes through with link 1 and no sigma
    rec = _Recorder()
    binary, _, _ = sc.fake_fit(0, family="binomial", n_chain=1, samplers=[rec])
    binary.predict_convergence(x, quantity="lik", y=(y > 0).astype(float))
    assert rec.calls[0]["link"] == 1 and rec.calls[0]["sigma"] is None and rec.calls[0]["peer_sigma"] is None and rec.calls[0]["peers"] == []


def test_python_refusals():
    fit, _, _ = sc.fake_fit(0, samplers=[_NoSampler(), _NoSampler()])
    x, y = np.zeros((40, 3)), np.zeros(40)
    with pytest.raises(ValueError, match="predict_convergence needs x_bart"):
        fit.predict_convergence()
    with pytest.raises(ValueError, match="quantity 'lik' needs y"):
        fit.predict_convergence(x, quantity="lik")
    with pytest.raises(ValueError, match="quantity 'ev' takes no y"):
        fit.predict_convergence(x, y=y)
    with pytest.raises(ValueError, match="quantity 'ev' takes no obs_weights"):
        fit.predict_convergence(x, obs_weights=np.ones(40))
    with pytest.raises(ValueError, match="'quantity' must be one of ev, lik"):
        fit.predict_convergence(x, quantity="ppd")
    with pytest.raises(ValueError, match="does not form 'ppd'"):
        fit.predict_convergence(x, type="ppd")
    with pytest.raises(ValueError, match="'type' must be one of ev, indiv.bart"):
        fit.predict_convergence(x, type="indiv.fixef")
    with pytest.raises(ValueError, match="'type' must be ev"):
        fit.predict_convergence(x, type="indiv.bart", quantity="lik", y=y)
    with pytest.raises(ValueError, match=r"y must have shape \[40\]"):
        fit.predict_convergence(x, quantity="lik", y=np.zeros(39))
    for bad in (np.zeros(40), np.full(40, np.inf), np.ones(39), -np.ones(40)):
        with pytest.raises(ValueError, match="obs_weights must be 40 finite values > 0"):
            fit.predict_convergence(x, quantity="lik", y=y, obs_weights=bad)
    for bad in (0.99, np.nan, (1.01, 1.05)):
        with pytest.raises(ValueError, match="'rhat_threshold' must be one value >= 1"):
            fit.predict_convergence(x, rhat_threshold=bad)
    bare, _, _ = sc.fake_fit(0)
    with pytest.raises(ValueError, match="predict_convergence requires 'bart_args' to contain 'keepTrees'"):
        bare.predict_convergence(x)
