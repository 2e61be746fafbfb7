"""s4b_predict_loo without a GPU: the sorted-row model of tests/loo_cases.py against a PAIRED transliteration (the proof that no draw index has to
travel through the sort), the generalised-Pareto fit on exact quantiles, the tail length by the integer rule, the share of rows the bound leaves out
on synthetic cases at the GPU tests' pool sizes, Stan4bartFit.predict_loo over stand-in samplers, every Python-side refusal, and the entry on the
emulated device layer (no such kernel there: refused with its message).  The kernel is tested in tests/test_gpu_predict_loo.py."""
import math
import os

import numpy as np
import pytest

import latent_par_cases as lp
import loo_cases as lc
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


def test_sorted_row_formula_against_the_paired_transliteration():
    """200 rows: 100 plain ones, 50 whose draws are tied in pairs and triples (inside the tail, across the cutoff and below it), 50 with a given
    tail.  The paired form puts the smoothed weight of rank j back at the draw that holds rank j (stable argsort) and sums l + lw over the DRAWS; the
    model sums over sorted positions and never knows a draw.  Both in long double: they agree to its rounding."""
    g = np.random.default_rng(11)
    worst = 0.0
    for rows, S, M, ties in ((100, 120, None, False), (50, 90, None, True), (50, 64, 31, True)):
        l = -0.5 * (g.normal(size=(rows, S)) * g.uniform(0.5, 3.0, (rows, 1))) ** 2
        if ties:
            l[:, 1::3] = l[:, 0:-1:3][:, :l[:, 1::3].shape[1]]          # pairs everywhere ...
            low = np.argsort(l, axis=1)[:, :5]                            # ... and the five LARGEST ratios (smallest l) all equal to the sixth: ties across the cutoff
            l[np.arange(rows)[:, None], low[:, :4]] = l[np.arange(rows), low[:, 4]][:, None]
        m = lc.tail_len(S) if M is None else M
        a = lc.psis(l, m)
        b, kb = lc.paired(l, m)
        assert np.array_equal(a["pareto_k"], kb)
        assert a["smoothed"].mean() > 0.9 and np.all(np.isfinite(b))
        if ties:
            srt = np.sort(-l, axis=1)
            assert np.all((np.diff(srt[:, S - m - 2:], axis=1) == 0).sum(axis=1) >= 3), "no tie reaches the tail"
        worst = max(worst, float(np.max(np.abs(a["elpd_loo"] - b) / (1.0 + np.abs(b)))))
    print(f"sorted-only against paired, 200 rows: max relative difference {worst:.3g}")
    assert worst <= 64 * float(np.finfo(LD).eps)


@pytest.mark.parametrize("k", [0.3, 0.7])
def test_gpd_fit_recovers_the_shape_of_exact_quantiles(k):
    N, sigma = 384, 1.7
    p = (np.arange(N).astype(LD) + LD(0.5)) / LD(N)
    x = LD(sigma) * np.expm1(-LD(k) * np.log1p(-p)) / LD(k)
    khat, sg = lc.gpd_fit(x[None, :])
    want = k * N / (N + 10) + 5.0 / (N + 10)
    print(f"GPD quantiles, k = {k}: khat {float(khat[0]):.4f} (prior-adjusted truth {want:.4f}), sigma {float(sg[0]):.4f}")
    assert abs(float(khat[0]) - want) <= 0.05 and abs(float(sg[0]) - sigma) <= 0.15 * sigma
    k64, _ = lc.gpd_fit(x[None, :], np.float64)
    assert abs(float(k64[0]) - float(khat[0])) < 1e-10


def test_tail_length_by_the_integer_rule():
    assert [lc.tail_len(S) for S in (20, 21, 25, 225, 226, 16384)] == [4, 5, 5, 45, 46, 384]
    assert [lc.tail_len(S) for S in (1, 2, 5, 6)] == [1, 1, 1, 2]
    for S in range(1, 16385, 37):          # the rule of the definition in floating point, where it is safe to form
        m = 3.0 * math.sqrt(S)
        if abs(m - round(m)) > 1e-9:
            assert lc.tail_len(S) == min(-(-S // 5), math.ceil(m)), S
    core = open(os.path.join(lp.CSRC, "sampler_core.hpp")).read()
    assert "while (m * m < 9 * S) ++m;" in core and "return std::min((S + 4) / 5, m);" in core
    src = open(os.path.join(lp.CSRC, "dev_loo.inc")).read()
    assert "const int W = R >= 4 ? 1 : 4 / R, slots = 4 / W;" in src and "for (int j = sub * 64 + lane; j < S; j += 64 * W)" in src          # (ppd_cases.tree_depth's geometry)
    assert "for (; j4 + 3 < M; j4 += 4)" in src and "for (int j = lane; j < M; j += 64) k0 +=" in src          # (loo_cases.fit_depth's)
    assert "constexpr int LOO_RED = 32;" in src and "(size_t)8 * LOO_RED + (size_t)8 * (size_t)slots * (size_t)c.tailLen" in src          # (loo_cases.lds_bytes)
    assert lc.lds_bytes(16384, 1024) == 131072 + 256 + 8192 <= 160 * 1024 and lc.lds_bytes(1024, 1023) == 32768 + 256 + 4 * 8184
    assert lc.fit_depth(384) == (98, 12)


@pytest.mark.parametrize("S,rows", [(21, 200), (64, 200), (65, 200), (1024, 50), (1025, 50), (2048, 50), (2049, 50), (4108, 50), (16380, 50)])
def test_synthetic_cases_stay_within_the_share_left_out(S, rows):
    """The model alone: the perturbed runs agree on the branch in all but 2 % of the rows (from_l asserts it), the heavy-tail regime is reached,
    and the tolerance is of the order the definition's conditioning predicts."""
    z, sigma, y = lc.synthetic(S, rows, 3)
    ref, bd, compared = lc.from_z(z, np.zeros_like(z), sigma, y, what=f"synthetic S {S}")
    k = ref["pareto_k"]
    assert (~compared).sum() <= 0.02 * rows and np.all(np.isfinite(k)) and k.max() > 0.7 and k.min() < 0.5
    assert np.all(ref["elpd_loo"] <= ref["lpd"] + 1e-12) and np.all(ref["ess"] >= 1.0 - 1e-12) and np.all(ref["ess"] <= S * (1 + 1e-12))
    for key in lc.OUTPUTS:
        assert np.all(bd[key] > 0) and np.all(bd[key][compared] < (1e-8 if key == "ess" else 1e-10)), (key, bd[key].max())
    print(f"synthetic S {S}: khat {k.min():.3g} .. {k.max():.3g}, largest bound " + ", ".join(f"{q} {bd[q].max():.3g}" for q in lc.OUTPUTS))


def test_model_branches_without_a_fit():
    g = np.random.default_rng(5)
    l = g.normal(size=(7, 20))
    a = lc.psis(l, lc.tail_len(20))          # M = 4: raw weights
    assert np.all(np.isinf(a["pareto_k"])) and not a["smoothed"].any()
    raw = -l.astype(LD)
    want = -(np.log(np.exp(raw).sum(axis=1)) - np.log(LD(20)))          # raw importance sampling: elpd = -log mean exp(-l)
    np.testing.assert_allclose(a["elpd_loo"].astype(np.float64), want.astype(np.float64), rtol=1e-14)
    const = lc.psis(np.full((3, 40), -1.25), 8)          # an equal tail
    assert np.all(np.isinf(const["pareto_k"])) and np.allclose(const["elpd_loo"].astype(np.float64), -1.25) and np.allclose(const["ess"].astype(np.float64), 40.0)
    one = lc.psis(l[:, :1], 1)
    assert np.array_equal(one["elpd_loo"].astype(np.float64), l[:, 0]) and np.array_equal(one["lpd"].astype(np.float64), l[:, 0])


def test_entry_is_refused_on_the_emulated_layer(emul_lib, emul_chain):
    assert hasattr(emul_lib, "emu_predict_loo")
    x = emul_chain.x[:7]
    for smp, S in ((emul_chain.live, 3), (emul_chain.stored[3], 3)):
        before = emul_chain.live.get_counters()
        with pytest.raises(RuntimeError, match="no PSIS-LOO kernels"):
            smp.predict_loo(x, y=np.zeros(7), sigma=np.ones(S))
        with pytest.raises(RuntimeError, match="no PSIS-LOO kernels"):
            smp.predict_loo(x, y=np.zeros(7), sigma=np.ones(S), peers=[emul_chain.stored[1]], peer_sigma=[np.ones(1)])
        assert not any(smp.loo_info.values()) and np.array_equal(emul_chain.live.get_counters(), before)
        with pytest.raises(ValueError, match="outputs must name at least one of"):
            smp.predict_loo(x, y=np.zeros(7), sigma=np.ones(S), outputs=())
        with pytest.raises(ValueError, match="outputs must name at least one of"):
            smp.predict_loo(x, y=np.zeros(7), sigma=np.ones(S), outputs=("elpd_loo", "pit"))
        with pytest.raises(ValueError, match=r"y must have shape \(7,\)"):
            smp.predict_loo(x, y=np.zeros(8), sigma=np.ones(S))
        with pytest.raises(ValueError, match=r"sigma must have shape \(3,\)"):
            smp.predict_loo(x, y=np.zeros(7), sigma=np.ones(4))
        with pytest.raises(ValueError, match=r"row_scale must have shape \(7,\)"):
            smp.predict_loo(x, y=np.zeros(7), sigma=np.ones(S), row_scale=np.ones(6))
        with pytest.raises(ValueError, match=r"peer_sigma\[0\] must be \[1 x 1\]"):
            smp.predict_loo(x, y=np.zeros(7), sigma=np.ones(S), peers=[emul_chain.stored[1]], peer_sigma=[np.ones(3)])


def test_oracle_library_has_no_entry(oracle_lib):
    from stan4bart_amd.abi import Sampler
    s = Sampler.__new__(Sampler)
    s._lib, s._pfx = oracle_lib, "orc_"
    with pytest.raises(RuntimeError, match="no predict_loo"):
        Sampler.predict_loo(s, np.zeros((2, 3)), y=np.zeros(2))


class _Recorder:
    """A stand-in sampler: records the call and answers with fixed per-row results."""

    def __init__(self, draws=15):
        self.calls, self.draws = [], draws

    def predict_loo(self, x, **kw):
        self.calls.append(dict(x=x, **kw))
        n = len(x)
        return dict(elpd_loo=-1.5 - 0.02 * np.arange(n), pareto_k=np.where(np.arange(n) % 4 == 0, np.inf, 0.05 * np.arange(n)), lpd=-1.0 - 0.01 * np.arange(n),
                    ess=np.full(n, 7.5), draws=self.draws, tail_len=kw.get("tail_len") or lc.tail_len(self.draws), info={})


class _NoSampler:
    def predict_loo(self, *a, **k):
        raise AssertionError("the ABI was called although the arguments had to be refused")


def test_fit_hands_sigma_per_chain_row_scale_and_the_tail_down():
    a, b, c = _Recorder(), _NoSampler(), _NoSampler()          # the first sampler takes the call, the others travel as its peers
    fit, new_terms, q = sc.fake_fit(0, n_chain=3, samplers=[a, b, c])
    g = np.random.default_rng(4)
    x, X, off, w, y = g.normal(size=(40, 3)), g.normal(size=(40, 2)), g.normal(size=40), g.uniform(0.5, 4.0, 40), g.normal(size=40)
    out = fit.predict_loo(x, X=X, groups=new_terms, offset=off, y=y, obs_weights=w, seed=5)
    assert len(a.calls) == 1
    call = a.calls[0]
    sig = fit.stan[fit.par_names.index("aux.1")]
    assert np.array_equal(call["sigma"], sig[:, 0]) and len(call["peer_sigma"]) == 2
    assert np.array_equal(call["peer_sigma"][0], sig[:, 1]) and np.array_equal(call["peer_sigma"][1], sig[:, 2])
    assert np.array_equal(call["row_scale"], 1.0 / np.sqrt(w)) and np.array_equal(call["y"], y) and call["link"] == 0 and call["peers"] == [b, c]
    assert call["tail_len"] == 0, "r_eff = 1 leaves the tail to the library's integer rule"
    linear = fit._summary_linear("ev", X, new_terms, off, True, np.random.default_rng(5))          # the same seed: predict's draws of unseen levels
    want = [linear(ch) for ch in range(3)]
    assert want[0]["ell_index"].max() >= q, "no unseen level reached the table"
    for key in ("offset", "dense", "dense_coef", "ell_index", "ell_value", "ell_coef"):
        assert np.array_equal(call[key], want[0][key]), key
    for ch in (1, 2):
        assert np.array_equal(call["peer_dense_coef"][ch - 1], want[ch]["dense_coef"]) and np.array_equal(call["peer_ell_coef"][ch - 1], want[ch]["ell_coef"])
    # what the host derives
    n = 40
    elpd, lpd, kk = -1.5 - 0.02 * np.arange(n), -1.0 - 0.01 * np.arange(n), np.where(np.arange(n) % 4 == 0, np.inf, 0.05 * np.arange(n))
    assert np.array_equal(out["elpd_loo"], elpd) and np.array_equal(out["lpd"], lpd) and np.array_equal(out["p_loo"], lpd - elpd)
    assert np.array_equal(out["pareto_k"], kk) and np.array_equal(out["ess"], np.full(n, 7.5))
    assert out["elpd_loo_total"] == float(elpd.sum()) and out["p_loo_total"] == float((lpd - elpd).sum())
    assert out["se"] == pytest.approx(math.sqrt(n * np.var(elpd, ddof=1)), rel=1e-14)
    thr = min(1.0 - 1.0 / math.log10(15), 0.7)
    assert out["k_threshold"] == pytest.approx(thr, rel=1e-15) and thr < 0.7 and out["n_high_k"] == int(np.sum(kk > thr)) and out["n_high_k"] >= 10
    assert out["draws"] == 15 and out["tail_len"] == lc.tail_len(15)
    big = _Recorder(draws=4000)
    fit2, _, _ = sc.fake_fit(1, n_iter=5, n_chain=1, samplers=[big])
    assert fit2.predict_loo(x, y=y)["k_threshold"] == 0.7 and big.calls[0]["row_scale"] is None and big.calls[0]["peers"] == [] and big.calls[0]["peer_sigma"] == []


def test_fit_turns_r_eff_into_a_tail_length_on_the_host():
    rec = _Recorder(draws=2000)
    fit, _, _ = sc.fake_fit(0, n_iter=1000, n_chain=2, samplers=[rec, _NoSampler()])
    x, y = np.zeros((6, 3)), np.zeros(6)
    for r_eff in (0.5, 0.25, 0.07):
        out = fit.predict_loo(x, y=y, r_eff=r_eff)
        want = math.ceil(min(2000 / 5.0, 3.0 * math.sqrt(2000 / r_eff)))
        assert rec.calls[-1]["tail_len"] == want == lc.tail_len_r_eff(2000, r_eff) == out["tail_len"] and lc.tail_len(2000) < want <= 400
    assert fit.predict_loo(x, y=y, r_eff=1.0)["tail_len"] == lc.tail_len(2000) == 135 and rec.calls[-1]["tail_len"] == 0
    small = _Recorder(draws=10)
    fit10, _, _ = sc.fake_fit(0, n_iter=5, n_chain=2, samplers=[small, _NoSampler()])
    fit10.predict_loo(x, y=y, r_eff=0.5)
    assert small.calls[-1]["tail_len"] == 0          # (fewer than 21 draws: no tail under any r_eff)
    many, _, _ = sc.fake_fit(0, n_iter=4000, n_chain=4, samplers=[_NoSampler()] * 4)
    with pytest.raises(ValueError, match="asks for a tail of 1200 of the 16000 draws: at most 1024"):
        many.predict_loo(x, y=y, r_eff=0.1)


def test_python_refusals():
    fit, _, _ = sc.fake_fit(0, samplers=[_NoSampler(), _NoSampler()])
    x, y = np.zeros((40, 3)), np.zeros(40)
    with pytest.raises(ValueError, match="predict_loo needs x_bart"):
        fit.predict_loo(y=y)
    with pytest.raises(ValueError, match="predict_loo needs y"):
        fit.predict_loo(x)
    with pytest.raises(ValueError, match=r"y must have shape \[40\]"):
        fit.predict_loo(x, y=np.zeros(39))
    for bad in (0.0, -0.5, 1.5, np.nan, (0.5, 0.5)):
        with pytest.raises(ValueError, match=r"'r_eff' must be one value in \(0, 1\]"):
            fit.predict_loo(x, y=y, r_eff=bad)
    for bad in (np.zeros(40), np.full(40, np.inf), np.ones(39), -np.ones(40)):
        with pytest.raises(ValueError, match="obs_weights must be 40 finite values > 0"):
            fit.predict_loo(x, y=y, obs_weights=bad)
    bare, _, _ = sc.fake_fit(0)
    with pytest.raises(ValueError, match="predict_loo requires 'bart_args' to contain 'keepTrees'"):
        bare.predict_loo(x, y=y)
    # a binary response goes through with link 1 and no sigma
    rec = _Recorder()
    binary, _, _ = sc.fake_fit(0, family="binomial", n_chain=1, samplers=[rec])
    out = binary.predict_loo(x, y=y)
    assert rec.calls[0]["link"] == 1 and rec.calls[0]["sigma"] is None and rec.calls[0]["peer_sigma"] is None and "elpd_loo" in out
    assert pp.C_HALF_LOG_2PI > 0.9          # (the likelihood is ppd_cases': imported, not restated)
