"""s4b_predict_check without a GPU: tests/check_cases.py's model against a brute-force loop over the replicate matrix (link 0 and link 1), the stated
order of the additions carried out in double against the model within the derived bounds, the shifted third moment against the raw form at a mean
of 1e6 and a spread of 1e-3, the assertion that no element of the cases is ambiguous, philox_uniform of philox.hpp against the model's, the refusal
on the emulated device layer and EVERY validation refusal through the emulated library (the checks run on every device layer, the launch does
not), the absence from the oracle library and the presence in the header.

No kernel runs here: the replicate, the model and the bounds are what tests/test_gpu_predict_check.py measures the device against."""
import os
import re
import subprocess

import numpy as np
import pytest

import check_cases as ck
import latent_par_cases as lp
import pd_cases as pc
import spread_cases as sp
from conftest import friedman_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS = (0.025, 0.5, 0.975, 0.0, 1.0)
KEY = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module")
def emul_chain(emul_lib):
    args, _ = friedman_case(n=100, T=5, warmup=3, iter=6, ranef=False)
    args.keep_trees = True
    c = pc.Chain(emul_lib, "emu_", args, steps=(1, 2), rows=300)
    yield c
    c.close()


def _inputs(ch, rows=300, link=0):
    """z [rows x 4] of the pool (3, 1) by the emulated layer's predict_bart, sigma, y, row_scale."""
    z = np.concatenate([ch.stored[3].predict_bart(ch.x), ch.stored[1].predict_bart(ch.x)], axis=1)[:rows]
    g = np.random.default_rng(17)
    if link:
        z = 1.5 * (z - z.mean()) / z.std()
        return z, None, (g.uniform(size=rows) < 0.5).astype(np.float64), None
    return z, g.uniform(0.5, 1.5, 4), z[:, 0] + g.normal(size=rows), g.uniform(0.5, 2.0, rows)


def _weights(kind, rows):
    if kind == "none":
        return None
    w = np.random.default_rng(1).uniform(0.0, 2.0, rows)
    if kind == "zero slab":
        w[128:256] = 0.0
    if kind == "indicator":
        w = (np.arange(rows) % 3 == 0).astype(np.float64)
        w[:128] = 0.0
    return w


@pytest.mark.parametrize("kind", ["none", "random", "zero slab", "indicator"])
@pytest.mark.parametrize("link, T", [(0, 0), (0, 1), (0, 5), (1, 0)])
def test_model_against_brute_force(emul_chain, kind, link, T):
    z, sigma, y, rs = _inputs(emul_chain, link=link)
    rows, S = z.shape
    w = _weights(kind, rows)
    rep = ck.replicate(z, 1e-18, sigma, KEY, rs, link)
    th = sp.thresholds_for(rep["x"], T, lo_inf=T >= 5, hi_inf=T >= 5)
    ref, bd = ck.model(z, 1e-18, y, sigma, KEY, w, th, PROBS, rs, link)
    assert ref["ambiguous"] == 0 and ref["draws"].shape == (7 + T, S) and ref["quantiles"].shape == (len(PROBS), 7 + T) and ref["observed"].shape == (5 + T,)
    # the replicate by a loop over the elements
    ww = np.ones(rows) if w is None else w
    x = np.zeros((rows, S))
    want_disc = np.zeros((2, S))
    for i in range(rows):
        for k in range(S):
            r = lp.philox4x32_10(i, 0, k, ck.ppd.PPD_TAG, KEY & 0xFFFFFFFF, KEY >> 32)
            u1, u2 = float(lp.u53(r[0], r[1])), float(lp.u53(r[2], r[3]))
            if link:
                Phi = float(ck.sc.phi_cdf(z[i, k]))
                x[i, k] = 1.0 if u1 <= Phi else 0.0
                want_disc[0, k] += -2.0 * ww[i] * np.log(Phi if x[i, k] else 1.0 - Phi)
                want_disc[1, k] += -2.0 * ww[i] * np.log(Phi if y[i] else 1.0 - Phi)
            else:
                e = np.sqrt(-2.0 * np.log(u1)) * np.cos(lp.TWO_PI * u2)
                sd = sigma[k] * rs[i]
                x[i, k] = z[i, k] + sd * e
                want_disc[0, k] += ww[i] * e * e
                want_disc[1, k] += ww[i] * ((y[i] - z[i, k]) / sd) ** 2
    np.testing.assert_allclose(ref["x"], x, rtol=1e-12, atol=1e-13)
    want = ck.brute_force(x, w, th)
    D = ref["draws"].astype(np.float64)
    np.testing.assert_allclose(D[:5 + T], want, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(D[5 + T:], want_disc / ww.sum(), rtol=1e-9 if not link else 1e-7)
    np.testing.assert_allclose(ref["observed"].astype(np.float64), ck.brute_force(y[:, None], w, th)[:, 0], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(ref["mean"], D.mean(axis=1), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(ref["quantiles"], np.quantile(D, PROBS, axis=1), rtol=1e-10, atol=1e-12)
    assert ref["weight"] == ck.gc.host_weight(ww) and ref["zero_slabs"] == (1 if kind in ("zero slab", "indicator") else 0)
    if w is None and T:
        assert np.all(bd["draws"][5:5 + T] == 0.0) and np.array_equal(D[5:5 + T], (x[:, :, None] > th[None, None, :]).sum(axis=0).T / float(rows))
    pv, pd = ck.p_values(D, ref["observed"].astype(np.float64), T)
    assert pv.shape == (5 + T,) and np.all((pv >= 0.0) & (pv <= 1.0)) and pd == np.mean(want_disc[0] >= want_disc[1])
    if link == 0:          # a threshold ON a replicate value is ambiguous
        r2, _ = ck.model(z, 1e-18, y, sigma, KEY, w, [float(ref["x"][7, 1])], (), rs, 0)
        assert r2["ambiguous"] >= 1


@pytest.mark.parametrize("kind", ["none", "random", "zero slab", "indicator"])
@pytest.mark.parametrize("rows", [1, 127, 128, 129, 300])
@pytest.mark.parametrize("link", [0, 1])
def test_stated_order_lies_within_the_bounds(emul_chain, kind, rows, link):
    """The header's order of the additions in plain double against the long-double model: within the derived bounds; the properties the header
    promises bit for bit hold for it."""
    z, sigma, y, rs = _inputs(emul_chain, rows, link)
    if not link:
        z, y = z + 40.0, y + 40.0          # (a mean far from 0 against the spread: what the shift is for)
    w = _weights(kind, 300)
    w = None if w is None else w[:rows]
    if w is not None and not w.sum() > 0.0:
        w[0] = 1.0
    rep = ck.replicate(z, 0.0, sigma, KEY, rs, link)
    T = 0 if link else 4
    th = () if link else (sp.thresholds_for(rep["x"], 4, lo_inf=True, hi_inf=True) if rows > 1 else np.array([-np.inf, np.inf]))
    T = len(th)
    ref, bd = ck.model(z, 0.0, y, sigma, KEY, w, th, (), rs, link)
    assert ref["ambiguous"] == 0
    xd = ref["x"]          # the replicate rounded to double: within bx of the model's
    if link:
        terms = (np.where(xd > 0.0, rep["l1"], rep["l0"]), np.where((y > 0.0)[:, None], rep["l1"], rep["l0"]))
    else:
        e = rep["e"].astype(np.float64)
        r = (y[:, None] - z) / rep["sd"]
        terms = (e * e, r * r)
    D = ck.device_order(xd, w, th, terms, link)
    parts = (("mean", slice(0, 1)), ("sd", slice(1, 2)), ("m3", slice(2, 3)), ("minmax", slice(3, 5)), ("share", slice(5, 5 + T)),
             ("disc_rep", slice(5 + T, 6 + T)), ("disc_obs", slice(6 + T, 7 + T)))
    ratios = {k: ck.bound_ratio(D[s], ref["draws"][s], bd["draws"][s]) for k, s in parts}
    obs = ck.device_order(y[:, None], w, th)[:, 0]
    ratios["observed"] = ck.bound_ratio(obs, ref["observed"], bd["observed"])
    print(f"{rows} rows, link {link}, weights {kind}: the stated order against the model, ratios to the bound {ratios}")
    assert all(v <= ck.BOUND_FACTOR for v in ratios.values()), ratios
    if T:
        assert np.all(D[5 + T - 1] == 0.0)          # t = +inf
        if w is None:
            assert np.all(D[5] == 1.0) and np.array_equal(D[5:5 + T], ref["draws"][5:5 + T].astype(np.float64))
    if rows == 1:
        assert np.array_equal(D[0], xd[0]) and np.all(D[1] == 0.0) and np.all(D[2] == 0.0) and np.array_equal(D[3], xd[0]) and np.array_equal(D[4], xd[0])
    if w is not None:
        assert np.array_equal(ck.device_order(xd, 2.0 * w, th, terms, link), D), "weights times 2 change an output"
    neg = ck.device_order(-xd, w, ())
    assert np.array_equal(neg[0], -D[0]) and np.array_equal(neg[1], D[1]) and np.array_equal(neg[2], -D[2]), "the mirrored replicate does not mirror the moments"


def test_raw_third_moment_would_not_meet_the_bound():
    """What the shift is for: at a mean of 1e6 and a spread of 1e-3 the raw third moment loses every digit, the stated order keeps it."""
    g = np.random.default_rng(0)
    x = 1e6 + 1e-3 * g.exponential(size=(300, 2))          # skewed: m3 is about 2e-9
    m3, b3 = ck.third_moment(x, 0.0)
    D = ck.device_order(x)
    assert ck.bound_ratio(D[2], m3, b3) <= ck.BOUND_FACTOR
    raw = np.array([ck.raw_third_moment(x[:, k]) for k in range(2)])
    assert ck.bound_ratio(raw, m3, b3) > 100.0
    assert np.all(b3 < 1e-2 * np.abs(m3).astype(np.float64)), "the bound of m3 says nothing at this shape"
    w = g.uniform(0.0, 2.0, 300)
    m3w, b3w = ck.third_moment(x, 0.0, w)
    assert ck.bound_ratio(ck.device_order(x, w)[2], m3w, b3w) <= ck.BOUND_FACTOR
    assert ck.bound_ratio([ck.raw_third_moment(x[:, k], w) for k in range(2)], m3w, b3w) > 100.0


def test_no_element_of_the_cases_is_ambiguous(emul_chain):
    """The CPU cases — the emulated chain's z under four keys, 64 thresholds from the reference replicate —: the reference alone shows that no uniform
    lies within its bound of Phi(z) and no replicate within its bound of a finite threshold; a uniform ON Phi(z) is counted.  The GPU cases have
    their own chains' z, which cannot be rebuilt here: for them the same count is asserted to be zero by check_cases.assert_check, in every case of
    tests/test_gpu_predict_check.py, from the reference alone and before anything of the device's is compared."""
    for link in (0, 1):
        z, sigma, y, rs = _inputs(emul_chain, link=link)
        for key in (KEY, 0, 7, 2 ** 64 - 1):
            rep = ck.replicate(z, 1e-15, sigma, key, rs, link)
            th = () if link else sp.thresholds_for(rep["x"], 64, True, True)
            ref, _ = ck.model(z, 1e-15, y, sigma, key, None, th, (), rs, link)
            assert ref["ambiguous"] == 0, (link, key)
    z, _, y, _ = _inputs(emul_chain, link=1)
    u = ck.uniform(KEY, np.arange(len(z)), np.arange(z.shape[1]))
    from statistics import NormalDist
    z2 = z.copy()
    z2[5, 2] = NormalDist().inv_cdf(float(u[5, 2]))          # Phi(z) on the uniform to within a few ulps
    assert ck.replicate(z2, 1e-15, None, KEY, None, 1)["ambiguous"] >= 1


def test_philox_uniform_of_the_header_is_the_models(tmp_path):
    """philox.hpp compiled on the host: philox_uniform is u53 of the first two words of philox_normal's block, and philox_normal is unchanged."""
    cxx = os.environ.get("CXX", "g++")
    src = tmp_path / "u.cpp"
    src.write_text('#include "philox.hpp"\n#include <cstdio>\n#include <initializer_list>\nint main() { const uint64_t key = 0x9E3779B97F4A7C15ull; '
                   'for (uint64_t r : {0ull, 5ull, 1099ull, (1ull << 32) + 3}) for (uint32_t d : {0u, 1u, 64u}) '
                   'std::printf("%a %a\\n", s4b::philox_uniform((uint32_t)key, (uint32_t)(key >> 32), r, d), s4b::philox_normal((uint32_t)key, (uint32_t)(key >> 32), r, d)); }\n')
    exe = tmp_path / "u"
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", lp.CSRC, "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split("\n")
    rows, draws = [0, 5, 1099, (1 << 32) + 3], [0, 1, 64]
    u = ck.uniform(KEY, rows, draws)
    e, be = ck.ppd.noise(KEY, rows, draws)
    for j, line in enumerate(out[:12]):
        gu, ge = (float.fromhex(t) for t in line.split())
        assert gu == u[j // 3, j % 3], (j, gu)
        assert abs(ge - float(e[j // 3, j % 3])) <= ck.BOUND_FACTOR * be[j // 3, j % 3]


def _args(ch, rows=7, **kw):
    z, sigma, y, rs = _inputs(ch, rows)
    a = dict(x_test=ch.x[:rows], y=y, sigma=np.full(3, 0.7), thresholds=(0.0,), probs=(0.5,))
    a.update(kw)
    return a


def test_entry_is_refused_on_the_emulated_layer(emul_lib, emul_chain):
    assert hasattr(emul_lib, "emu_predict_check")
    for smp in (emul_chain.live, emul_chain.stored[3]):
        assert smp.check_draws() == 3
        before = emul_chain.live.get_counters()
        with pytest.raises(RuntimeError, match="predict_check: this device layer has no check kernels"):
            smp.predict_check(**_args(emul_chain))
        with pytest.raises(RuntimeError, match="no check kernels"):
            smp.predict_check(**_args(emul_chain, weights=np.ones(7), peers=[emul_chain.stored[1]], peer_sigma=[np.ones(1)], row_scale=np.ones(7)))
        with pytest.raises(RuntimeError, match="no check kernels"):
            smp.predict_check(**_args(emul_chain, link=1, thresholds=(), sigma=None, y=np.arange(7.0) % 2))
        assert not any(smp.check_info.values()) and np.array_equal(emul_chain.live.get_counters(), before)
        with pytest.raises(RuntimeError, match="no spread kernels"):          # the sibling's refusal is what it was
            smp.predict_spread(emul_chain.x[:7])


REFUSALS = [
    (r"predict_check: n_thresholds must lie in \[0, 64\], not 65", dict(thresholds=np.arange(65.0))),
    ("predict_check: n_thresholds must be 0 under link 1", dict(link=1, sigma=None, y=np.arange(7.0) % 2)),
    ("predict_check: threshold 1 is a NaN", dict(thresholds=(0.0, np.nan))),
    ("predict_check: the thresholds are not strictly ascending at index 2", dict(thresholds=(0.0, 1.0, 1.0))),
    ("predict_check: the thresholds are not strictly ascending at index 1", dict(thresholds=(np.inf, np.inf))),
    ("predict_check: the thresholds are not strictly ascending at index 1", dict(thresholds=(1.0, -1.0))),
    ("predict_check: bin_index must be 0 .*, not 3", dict(bin_index=3)),
    ("predict_check: between 0 and 16 probs per call, not 17", dict(probs=np.linspace(0.0, 1.0, 17))),
    ("predict_check: prob 1.5.* outside", dict(probs=(1.5,))),
    ("predict_check: negative scratch_bytes", dict(scratch_bytes=-1)),
    ("predict_check: NULL y", dict(y=None)),
    ("predict_check: weight -1.* of row 3 is negative or not finite", dict(weights=np.r_[1.0, 1.0, 1.0, -1.0, 1.0, 1.0, 1.0])),
    ("predict_check: weight nan.* of row 3 is negative or not finite", dict(weights=np.r_[1.0, 1.0, 1.0, np.nan, 1.0, 1.0, 1.0])),
    ("predict_check: weight inf.* of row 3 is negative or not finite", dict(weights=np.r_[1.0, 1.0, 1.0, np.inf, 1.0, 1.0, 1.0])),
    ("predict_check: the weights sum to 0", dict(weights=np.zeros(7))),
    ("predict_check: link 0 needs sigma", dict(sigma=None)),
    ("predict_check: sigma holds 0.* at draw 1", dict(sigma=np.r_[1.0, 0.0, 1.0])),
    ("predict_check: sigma holds nan.* at draw 2", dict(sigma=np.r_[1.0, 1.0, np.nan])),
    ("predict_check: row_scale holds -1.* at row 2", dict(row_scale=np.r_[1.0, 1.0, -1.0, 1.0, 1.0, 1.0, 1.0])),
    ("predict_check: row_scale is 0 at row 2", dict(row_scale=np.r_[1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0])),
    ("predict_check: y holds nan.* at row 4", dict(y=np.r_[0.0, 0.0, 0.0, 0.0, np.nan, 0.0, 0.0])),
    ("predict_check: y holds inf.* at row 4", dict(y=np.r_[0.0, 0.0, 0.0, 0.0, np.inf, 0.0, 0.0])),
    ("predict_check: y holds 2.* at row 4: under link 1 every y is 0 or 1", dict(link=1, thresholds=(), sigma=None, y=np.r_[0.0, 1.0, 0.0, 1.0, 2.0, 0.0, 1.0])),
    ("predict_check: link 0 needs peer_sigma", dict(peers="one")),
]


@pytest.mark.parametrize("match, kw", REFUSALS, ids=[f"{j}: {m[15:50]}" for j, (m, _) in enumerate(REFUSALS)])
def test_every_validation_refusal_through_the_emulated_library(emul_chain, match, kw):
    """The checks of s4b_predict_check run before the device layer is asked: the emulated library refuses every invalid call with the check's own
    message, leaves info zero and launches nothing."""
    kw = dict(kw)
    if kw.get("peers") == "one":
        kw["peers"] = [emul_chain.stored[1]]
    for smp in (emul_chain.live, emul_chain.stored[3]):
        before = emul_chain.live.get_counters()
        with pytest.raises(RuntimeError, match=match):
            smp.predict_check(**_args(emul_chain, **kw))
        assert not any(smp.check_info.values()), smp.check_info
        assert np.array_equal(emul_chain.live.get_counters(), before), "a refused call launched something"


def test_binding_refusals_and_names(emul_chain):
    from stan4bart_amd.abi import CHECK_INFO, Sampler
    assert len(CHECK_INFO) == 8 and Sampler.check_names(2) == ck.names(2) == ["mean", "sd", "m3", "min", "max", "share_above[0]", "share_above[1]", "disc_rep", "disc_obs"]
    smp = emul_chain.stored[3]
    for match, kw in (("unknown outputs", dict(outputs=("p_value",))), ("thresholds must be a vector", dict(thresholds=np.zeros((2, 2)))),
                      (r"weights must have shape \(7,\)", dict(weights=np.ones(6))), (r"y must have shape \(7,\)", dict(y=np.ones(8))),
                      ("bin_index must be one of auto, compare, search", dict(bin_index="bisect")), ("probs must be a vector", dict(probs=np.zeros((2, 2))))):
        with pytest.raises(ValueError, match=match):
            smp.predict_check(**_args(emul_chain, **kw))


def test_oracle_library_has_no_entry_and_the_header_has_it(oracle_lib):
    from stan4bart_amd.abi import Sampler
    assert not hasattr(oracle_lib, "orc_predict_check")
    s = Sampler.__new__(Sampler)
    s._lib, s._pfx = oracle_lib, "orc_"
    with pytest.raises(RuntimeError, match="no predict_check"):
        Sampler.predict_check(s, np.zeros((2, 3)))
    header = open(os.path.join(ROOT, "include", "stan4bart_amd.h")).read()
    assert re.search(r"int S4B_FN\(predict_check\)\(s4b_sampler\* s, const s4b_check_in\* in, s4b_check_out\* out\);", header)
    for said in ("THE ORDER OF THE ADDITIONS", "the shift c = the replicate of the slab's first row", "M3_s = (s3 - 3 d s2) + 2 d^2 s1",
                 "delta^3 W_a W_b (W_a - W_b) / W_ab^2 + 3 delta (W_a M2_b - W_b M2_a) / W_ab", "from b = T downward", "A partial with W_s = 0 is skipped",
                 "FIRST TWO words of the same Philox block", "THE SAME BITS predict_ppd sorts"):
        assert said in header, said


class _Recorder:
    """A stand-in sampler of 10 draws per chain: records the call and answers with a matrix the views can be checked on."""

    def __init__(self, draws=10):
        self.calls, self.draws = [], draws

    def predict_check(self, x, **kw):
        self.calls.append(kw)
        T, Q, S = len(kw["thresholds"]), len(kw["probs"]), self.draws * (1 + len(kw["peers"]))
        k = np.arange(S, dtype=np.float64)
        D = np.zeros((7 + T, S))
        D[0], D[1], D[2], D[3], D[4] = 2.0 + k, 0.5 + 0.25 * k, 0.125 * (k - 3.0), -1.0 - k, 9.0
        D[1, 4] = 0.0          # a draw without spread: its skewness is NaN
        for j in range(T):
            D[5 + j] = (k % (j + 2)) / 4.0
        D[5 + T], D[6 + T] = 1.0 + 0.1 * k, 2.0
        obs = np.r_[5.0, 1.0, 0.25, -3.0, 9.0, np.full(T, 0.25)]
        return dict(draws=D, observed=obs, mean=D.mean(axis=1), m2=((D - D.mean(axis=1, keepdims=True)) ** 2).sum(axis=1),
                    quantiles=np.quantile(D, kw["probs"], axis=1) if Q else None, names=ck.names(T), weight=3.5, thresholds=np.asarray(kw["thresholds"]),
                    draws_pooled=S, info={"thresholds": T})


def _fit(samplers, family="gaussian", iters=10):
    from stan4bart_amd.generics import Stan4bartFit
    fit = Stan4bartFit.__new__(Stan4bartFit)
    fit.samplers, fit.family = samplers, family
    fit.par_names = ["aux.1"]
    fit.stan = np.arange(1.0, 1.0 + iters * len(samplers)).reshape(len(samplers), iters).T[None, :, :]          # [par, iter, chain]
    fit._summary_linear = lambda *a, **k: (lambda c: dict(offset=None, dense=None, dense_coef=None, ell_index=None, ell_value=None, ell_coef=None))
    return fit


def test_views_p_values_and_the_pooled_call():
    rec = _Recorder()
    fit = _fit([rec, object()])
    x, y = np.zeros((6, 3)), np.arange(6.0)
    out = fit.pp_check(x_bart=x, y=y, thresholds=(0.0, 1.0), row_weights=np.ones(6), obs_weights=np.full(6, 4.0), probs=(0.25, 0.75), seed=11, return_draws=True)
    call = rec.calls[-1]
    assert len(call["peers"]) == 1 and np.array_equal(call["sigma"], np.arange(1.0, 11.0)) and np.array_equal(call["peer_sigma"][0], np.arange(11.0, 21.0))
    assert np.array_equal(call["row_scale"], np.full(6, 0.5)) and np.array_equal(call["weights"], np.ones(6)) and np.array_equal(call["y"], y)
    ss = np.random.SeedSequence(11)
    assert out["noise_key"] == call["noise_key"] == int(ss.generate_state(1, np.uint64)[0]) and out["seed"] == 11 and out["draws"] == 20
    D = out["matrix"]
    assert out["mean"]["observed"] == 5.0 and out["mean"]["p_value"] == np.mean(D[0] >= 5.0) and np.array_equal(out["mean"]["draws"], D[0])
    assert out["min"]["p_value"] == 0.15 and out["max"]["p_value"] == 1.0          # >=: a tie counts (min: draws 0, 1, 2 of 20)
    assert out["sd"]["sd"] == pytest.approx(D[1].std(ddof=1)) and np.array_equal(out["sd"]["quantiles"], np.quantile(D[1], (0.25, 0.75)))
    assert len(out["share_above"]) == 2 and out["share_above"][1]["p_value"] == np.mean(D[6] >= 0.25)
    sk = out["skewness"]
    assert np.isnan(sk["draws"][4]) and sk["draws"][7] == D[2, 7] / D[1, 7] ** 3 and sk["observed"] == 0.25 and np.isnan(sk["mean"])
    assert sk["p_value"] == np.mean(np.nan_to_num(sk["draws"], nan=-np.inf) >= 0.25)
    assert out["discrepancy"]["p_value"] == np.mean(D[7] >= D[8]) == 0.5 and out["discrepancy"]["observed"] == 2.0
    brief = fit.pp_check(x_bart=x, y=y, seed=11)
    assert "matrix" not in brief and "draws" not in brief["mean"] and brief["share_above"] == [] and brief["noise_key"] == out["noise_key"]
    assert rec.calls[-1]["row_scale"] is None and rec.calls[-1]["weights"] is None
    other = fit.pp_check(x_bart=x, y=y, seed=12)
    assert other["noise_key"] != out["noise_key"]
    # a binary fit hands no sigma down and takes no thresholds
    fb = _fit([rec], family="binomial")
    fb.pp_check(x_bart=x, y=np.arange(6.0) % 2, seed=1)
    assert rec.calls[-1]["sigma"] is None and rec.calls[-1]["peer_sigma"] is None
    for match, kw in (("takes no thresholds for a binary response", dict(thresholds=(0.5,))), ("y must be 0 or 1", dict(y=np.arange(6.0)))):
        with pytest.raises(ValueError, match=match):
            fb.pp_check(**dict(dict(x_bart=x, y=np.arange(6.0) % 2), **kw))
    for match, kw in (("needs y", dict(y=None)), ("needs x_bart", dict(x_bart=None)), ("y must be 6 finite", dict(y=np.ones(5))), ("strictly ascending", dict(thresholds=(1.0, 1.0))),
                      ("row_weights sum to 0", dict(row_weights=np.zeros(6))), ("row_weights must be", dict(row_weights=-np.ones(6))),
                      ("obs_weights must be", dict(obs_weights=np.zeros(6))), ("'probs' must be", dict(probs=(2.0,))),
                      ("at most 64", dict(thresholds=np.arange(65.0)))):
        with pytest.raises(ValueError, match=match):
            fit.pp_check(**dict(dict(x_bart=x, y=y), **kw))
    with pytest.raises(ValueError, match="keepTrees"):
        _fit([]).pp_check(x_bart=x, y=y)
