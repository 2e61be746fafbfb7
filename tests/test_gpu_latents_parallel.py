"""Latent mode "parallel" (bart_args latents, s4b_set_latent_mode 1, k_latents_par) on the MI355X: the latents are exactly truncated normal given
the sampler's own means, the chain is the same on every tree path, from run to run, through get_state / set_state and in sweep groups, the
posterior agrees with the exact mode's, and the draw is far faster than R's stream.  This mode is a different chain from the reference's: nothing
here is compared with the oracle."""
import copy

import numpy as np
import pytest
from scipy import stats

from conftest import StateView, make_sampler, run_chain

pytestmark = pytest.mark.gpu


def _data(n, seed=0):
    from stan4bart_amd import GroupTerm
    g = np.random.default_rng(700 + seed)
    xb = np.asfortranarray(g.random((n, 5)))
    X = g.random((n, 1))
    grp = g.integers(1, 9, size=n)
    b = 0.7 * g.standard_normal(9)
    eta = 1.5 * np.sin(np.pi * xb[:, 0] * xb[:, 1]) + 2.0 * (xb[:, 2] - 0.5) + (X[:, 0] - 0.5) + b[grp]
    y = (eta + g.standard_normal(n) > 0.0).astype(np.float64)
    return y, xb, X, [GroupTerm(grp, None, "g.1")]


def _case(n, seed=0, trees=10, iters=(2, 6), latents="parallel", offset=None, y=None, k=None):
    from stan4bart_amd import make_sampler_args
    y0, xb, X, groups = _data(n, seed)
    bart = {"n.trees": trees, "latents": latents}
    if k is not None:
        bart["k"] = k
    return make_sampler_args(y0 if y is None else y, xb, X=X, groups=groups, family="binomial", iter=iters[1], warmup=iters[0],
                             offset=offset, bart_args=bart)


def _lat_fields(blob):
    """(mean, R, mode) of the latent draw that ended the iteration: mean = tree fits + offset, R = z - mean (k_latents_finish's conventions)."""
    mode = int(np.frombuffer(blob, dtype=np.int64, count=1, offset=40)[0])
    sv = StateView(blob[:-16] if mode == 1 else blob)
    off, fits, lat = sv.get("offset"), sv.get("total_fits"), sv.get("latents")
    return off + fits, (lat + off) - (off + fits), mode


def _tail(blob):
    return np.frombuffer(blob[-16:], dtype=np.uint64)


def _uniforms(mean, R, y):
    """P(X >= R | X >= -mean) for y = 1, P(X <= R | X <= -mean) for y = 0: uniform if R is N(0, 1) truncated by y (log survival functions:
    the far tails are not 1 - Phi)."""
    lo = np.exp(stats.norm.logcdf(R) - stats.norm.logcdf(-mean))
    hi = np.exp(stats.norm.logsf(R) - stats.norm.logsf(-mean))
    return np.where(y > 0, hi, lo)


@pytest.mark.parametrize("latents", ["exact", "parallel"])
def test_latents_are_exactly_truncated_normal(hip_lib, latents):
    """1e6 latents (250 000 observations x 4 iterations) through a real sampler; a user offset spreads the means over [-8, 8] and y is drawn
    independently of it, so both rejection branches run and deep tails occur.  The exact path passes the same check (the harness is sound)."""
    n, iters = 250_000, 4
    g = np.random.default_rng(17)
    offset = g.uniform(-8.0, 8.0, n)
    y = (g.random(n) < 0.5).astype(np.float64)
    s = make_sampler(hip_lib, "s4b_", _case(n, seed=1, trees=5, latents=latents, offset=offset, y=y), seed=4242)
    try:
        assert s.get_latent_mode() == (1 if latents == "parallel" else 0)
        us, lowers = [], []
        for _ in range(iters):
            s.run(1, True, 1)
            mean, R, mode = _lat_fields(s.get_state())
            assert mode == s.get_latent_mode()
            assert np.all(np.isfinite(R)) and np.all(np.where(y > 0, R >= -mean, R <= -mean))
            us.append(_uniforms(mean, R, y))
            lowers.append(np.where(y > 0, -mean, mean))
    finally:
        s.free()
    u, lower = np.concatenate(us), np.concatenate(lowers)
    assert u.size >= 1_000_000 and (lower < 0).sum() > 100_000 and (lower >= 4).sum() > 100_000
    for name, sel in (("all", slice(None)), ("normal branch", lower < 0), ("exponential branch", lower >= 0), ("lower >= 6", lower >= 6)):
        p = stats.kstest(u[sel], "uniform").pvalue
        assert p > 1e-3, (latents, name, p)


def _same(a, b, exact=True):
    assert np.array_equal(a["trace"], b["trace"]), "tree-move trace differs"
    assert np.array_equal(a["rng"], b["rng"]), "R generator state differs"
    for ph in ("warmup", "sample"):
        for x, z in ((a[ph]["bart"]["train"], b[ph]["bart"]["train"]), (a[ph]["stan"], b[ph]["stan"])):
            if exact:
                assert np.array_equal(x, z), ph
            else:
                np.testing.assert_allclose(x, z, rtol=1e-9, atol=1e-12, err_msg=ph)


@pytest.mark.parametrize("k", [None, ("chi", 1.25, float("inf"))], ids=["fixed-k", "modeled-k"])
def test_parallel_chain_is_the_same_on_every_tree_path(hip_lib, k):
    """Persistent, fused and two-kernel tree updates, the persistent path's busy fallback (test hook), run to run: the same chain.  Run to run
    it is bit for bit; across paths the tree fits differ only in the summation order of the bin sums (1e-15 relative, as in the exact mode),
    so the moves and R's stream are identical and the values agree to 1e-9."""
    args = _case(6000, seed=2, trees=20, iters=(4, 10), k=k)       # (more than one workgroup: the busy hook needs a roll call)
    base = run_chain(hip_lib, "s4b_", args, tree_path="persistent")
    assert base["tree_path"] == ("persistent", "persistent")
    _same(base, run_chain(hip_lib, "s4b_", args, tree_path="persistent"))
    for path in ("fused", "two-kernel"):
        r = run_chain(hip_lib, "s4b_", args, tree_path=path)
        assert r["tree_path"] == (path, path)
        _same(base, r, exact=False)
    busy = run_chain(hip_lib, "s4b_", args, tree_path="persistent", test_hook=(1, 3))
    assert busy["sweep_busy"] > 0
    _same(base, busy, exact=False)
    ex = copy.copy(args)
    ex.latents = "exact"
    assert not np.array_equal(run_chain(hip_lib, "s4b_", ex, tree_path="persistent")["rng"], base["rng"]), "the latents still draw from R's stream"


def test_state_round_trip_and_mode_check(hip_lib):
    args = _case(2000, seed=3, trees=15, iters=(3, 9))
    a = make_sampler(hip_lib, "s4b_", args)
    b = make_sampler(hip_lib, "s4b_", args)
    ex = copy.copy(args)
    ex.latents = "exact"
    c = make_sampler(hip_lib, "s4b_", ex)
    other = make_sampler(hip_lib, "s4b_", args, seed=999)
    try:
        a.run(3, True)
        blob = a.get_state()
        key, draws = _tail(blob)
        assert draws == 3 and key != 0
        other.run(1, True)
        assert _tail(other.get_state())[0] != key, "different seeds gave the same Philox key"
        ra = a.run(5, True)
        b.set_state(blob)
        rb = b.run(5, True)
        assert np.array_equal(ra["bart"]["train"], rb["bart"]["train"]) and np.array_equal(ra["stan"], rb["stan"])
        assert a.get_state() == b.get_state()
        c.run(1, True)
        before = c.get_state()
        with pytest.raises(RuntimeError, match="latent mode"):
            c.set_state(blob)
        assert c.get_state() == before
        with pytest.raises(RuntimeError, match="latent mode"):
            b.set_state(before)
        with pytest.raises(RuntimeError, match="before the first run"):
            c.set_latent_mode(1)
    finally:
        for s in (a, b, c, other):
            s.free()


def test_batched_chains_draw_what_unbatched_chains_draw(hip_lib):
    from stan4bart_amd import stan4bart
    y, xb, X, groups = _data(1500, seed=4)
    kw = dict(X=X, groups=groups, family="binomial", chains=4, cores=4, seed=11, iter=16, warmup=8, bart_args={"n.trees": 20, "latents": "parallel"})
    f1 = stan4bart(y, xb, batch_chains=False, **kw)
    f2 = stan4bart(y, xb, batch_chains=True, **kw)
    assert f1.latents == f2.latents == "parallel"
    assert f2.batch_stats["batched_sweeps"] > 0, f2.batch_stats
    assert np.array_equal(f1.bart_train, f2.bart_train) and np.array_equal(f1.stan, f2.stan)


def test_posterior_agrees_with_the_exact_mode(hip_lib):
    """Probit with a random intercept, n = 5 000, 4 chains each: per-observation posterior mean probabilities and the random-intercept SD.
    The tolerance is what two exact-mode fits with different seeds differ by."""
    from stan4bart_amd import stan4bart
    y, xb, X, groups = _data(5000, seed=5)

    def fit(latents, seed):
        f = stan4bart(y, xb, X=X, groups=groups, family="binomial", chains=4, cores=4,
                      seed=seed, iter=400, warmup=200, bart_args={"n.trees": 50, "latents": latents})
        sd = float(np.sqrt(np.mean(f.extract("Sigma")["g.1"][0, 0])))
        return f.fitted("ev"), sd
    pa, sa = fit("exact", 1)
    pb, sb = fit("exact", 2)
    pp, sp = fit("parallel", 3)
    ref = np.mean(np.abs(pa - pb))
    assert np.mean(np.abs(pp - pa)) < 2.0 * ref, (np.mean(np.abs(pp - pa)), ref)
    assert np.max(np.abs(pp - pa)) < 3.0 * np.max(np.abs(pb - pa)) + 0.01
    assert abs(sp - sa) < max(3.0 * abs(sb - sa), 0.15 * sa), (sa, sb, sp)


def test_parallel_latents_are_far_faster_at_one_million(hip_lib):
    import time
    rates = {}
    for latents in ("exact", "parallel"):
        s = make_sampler(hip_lib, "s4b_", _case(1_000_000, seed=6, trees=4, latents=latents))
        try:
            s.run(1, True, 1)
            t0 = time.perf_counter()
            s.run(4, True, 1)
            rates[latents] = 4 / (time.perf_counter() - t0)
        finally:
            s.free()
    assert rates["parallel"] >= 10.0 * rates["exact"], rates
