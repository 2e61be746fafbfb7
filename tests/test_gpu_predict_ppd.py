"""s4b_predict_ppd on the device (stan4bart_amd/csrc/dev_ppd.inc: k_predict_values<staged / global> unchanged, k_ppd_rows) against numpy on the full pooled
matrix (tests/ppd_cases.py: the model and the derived bounds).  Pooled draw counts 1, 2, 5, 13, 5 + 13 and 5 x 13 on both routes with dense and ELL
parts, an offset and a sigma table per peer; the anchor to k_row_quantiles (row_scale 0: the same bits); the rows per workgroup around their count,
one row per workgroup up to the LDS maximum; chunks, live and stored samplers, determinism, the noise key; a binary response; the extremes of the
scores; the refusals before any launch; the whole Python interface.

One small Friedman chain per response kind (n = 400, T <= 25, a dozen iterations), built as pd_cases.Chain builds them; samplers with fewer draws are
stored samplers rebuilt from states exported while the chain ran.  The BART fits of the reference are computed once per sampler."""
import struct

import numpy as np
import pytest

import pd_cases as pc
import ppd_cases as pp
import readout_cases as rc
import summary_cases as sc

pytestmark = pytest.mark.gpu
POOLS = {1: (1,), 2: (2,), 5: (5,), 13: (13,), 18: (5, 13), 65: (13,) * 5}          # pooled draws -> the stored samplers pooled, the first takes the call
PROBS = (0.025, 0.5, 0.975, 0.0, 1.0, 1.0 / 3.0)
KEY = 0x6A09E667F3BCC908
SCORES = ("lpd", "lmean", "lm2", "pit")


def _report(line):
    print(line)


class Chain(pc.Chain):
    """pd_cases.Chain on the product library, with predict_bart of every stored sampler at its rows (computed when first asked for)."""

    def __init__(self, lib, args, rows):
        super().__init__(lib, "s4b_", args, rows=rows)
        self._bart = {}

    def bart(self, S):
        if S not in self._bart:
            self._bart[S] = self.stored[S].predict_bart(self.x)
        return self._bart[S]


@pytest.fixture(scope="module")
def gauss(hip_lib):
    c = Chain(hip_lib, rc._friedman(n=400, T=25, warmup=4, iter=17, ranef=False), rows=1100)
    yield c
    c.close()


@pytest.fixture(scope="module")
def binary(hip_lib):
    c = Chain(hip_lib, rc._binary(n=400, T=11, warmup=6, iter=19), rows=400)
    yield c
    c.close()


def _sigma(S, j, seed):
    return np.random.default_rng([9000, seed, j, S]).uniform(0.5, 2.0, S)


def _inputs(chain, pool, rows, M=0, E=0, offset=False, seed=0):
    """The arguments of a pooled call over the first `rows` rows and the model's `parts`: the row side (dense, ELL entries, offset) is shared, every
    pooled sampler gets coefficient tables and a sigma vector of its own."""
    x = np.asfortranarray(chain.x[:rows])
    shared = sc.linear_parts(rows, pool[0], M, E, seed=seed)
    tables = [shared] + [sc.linear_parts(rows, S, M, E, seed=seed + 100 + j) for j, S in enumerate(pool[1:])]
    sigmas = [_sigma(S, j, seed) for j, S in enumerate(pool)]
    off = 3.0 * np.random.default_rng(seed).uniform(-1.0, 1.0, rows) if offset else None
    kw = dict(offset=off, peers=[chain.stored[S] for S in pool[1:]], sigma=sigmas[0], peer_sigma=sigmas[1:], **shared)
    if M:
        kw["peer_dense_coef"] = [t["dense_coef"] for t in tables[1:]]
    if E:
        kw["peer_ell_coef"] = [t["ell_coef"] for t in tables[1:]]
    parts = [dict(bart=chain.bart(S)[:rows], sigma=sg, dense_coef=t.get("dense_coef"), ell_coef=t.get("ell_coef")) for S, t, sg in zip(pool, tables, sigmas)]
    row_side = dict(offset=off, dense=shared.get("dense"), ell_index=shared.get("ell_index"), ell_value=shared.get("ell_value"))
    return x, kw, parts, row_side


def _responses(parts, row_side, seed):
    """Held-out responses a few sd around the rows' predictions."""
    z, _ = pp.pooled_z(parts, **row_side)
    return z.mean(axis=1) + 1.5 * np.random.default_rng([7000, seed]).standard_normal(len(z))


def _row_scale(rows, seed):
    return np.random.default_rng([8000, seed]).uniform(0.25, 3.0, rows)


_REF = {}


def _case(chain, pool, rows, what, probs=PROBS, scored=True, scaled=True, M=0, E=0, offset=False, seed=0, key=KEY, **call):
    """One pooled call against the model; the reference of a case is computed once and shared by the routes."""
    x, kw, parts, row_side = _inputs(chain, pool, rows, M, E, offset, seed)
    y = _responses(parts, row_side, seed) if scored else None
    rs = _row_scale(rows, seed) if scaled else None
    got = chain.stored[pool[0]].predict_ppd(x, probs, y=y, row_scale=rs, noise_key=key, **kw, **call)
    S = sum(pool)
    assert got["draws"] == S and got["info"]["draws"] == S and got["info"]["launches"] == 2 * got["info"]["chunks"]
    ck = (id(chain), pool, rows, tuple(probs), scored, scaled, M, E, offset, seed, key)
    if ck not in _REF:
        _REF[ck] = pp.model(parts, key, probs, y=y, row_scale=rs, **row_side)
    ref, bd = _REF[ck]
    pp.assert_ppd(got, ref, bd, what, _report)
    return got, (x, dict(kw, y=y, row_scale=rs, noise_key=key)), (parts, row_side)


def _same_bits(a, b, what, keys=("quantiles",) + SCORES):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            assert np.array_equal(a[k], b[k]), f"{what}: {k} differs"


@pytest.mark.parametrize("S", sorted(POOLS))
def test_pooled_draw_counts_against_the_model_on_both_routes(gauss, S):
    pool, rows = POOLS[S], 700
    for what, opt in (("quantiles alone, no row_scale", dict(scored=False, scaled=False)), ("quantiles and scores", dict()),
                      ("scores alone", dict(probs=()))):
        res = {}
        for route in ("staged", "global"):
            res[route], _, (parts, row_side) = _case(gauss, pool, rows, f"S {S} {route}, {what}", M=2, E=2, offset=True, seed=S, route=route, **opt)
            info = res[route]["info"]
            sp = 1 << (S - 1).bit_length()
            assert info["route"] == (1 if route == "staged" else 2) and info["padded_draws"] == sp and info["rows_per_sort"] == 4096 // sp
            assert info["rows_per_chunk"] == rows and info["chunks"] == 1
        _same_bits(res["staged"], res["global"], f"S {S}, {what}: the two routes")
    alone = res["staged"]          # (the scores of the call without quantiles)
    if len(pool) > 1:          # every peer's own sigma reached its draws: the model with the first table for all is another answer
        got, _, (parts, row_side) = _case(gauss, pool, rows, f"S {S}, per-peer sigma", M=2, E=2, offset=True, seed=S)
        same = [dict(p, sigma=np.resize(parts[0]["sigma"], len(p["sigma"]))) for p in parts]
        y, rs = _responses(parts, row_side, S), _row_scale(rows, S)
        other, bd = pp.model(same, KEY, PROBS, y=y, row_scale=rs, **row_side)
        assert pp.bound_ratio(got["quantiles"], other["quantiles"], bd["quantiles"]) > 1e6 and pp.bound_ratio(got["lpd"], other["lpd"], bd["lpd"]) > 1e6, \
            "the peers' sigma vectors do not matter: the case tests no per-peer sigma"
        _same_bits(got, alone, "the scores with and without quantiles", SCORES)


@pytest.mark.parametrize("S", sorted(POOLS))
def test_zero_row_scale_returns_the_bits_of_predict_quantiles(gauss, S):
    """sd = 0: y_rep = z + 0 e = z, and the sort and the interpolation are the functions k_row_quantiles calls.  (z + 0 e is z bit for bit except
    that a z of -0.0 comes out as +0.0 where e > 0; np.array_equal takes the two zeros for equal, and no z of these cases is a zero.)"""
    pool, rows = POOLS[S], 700
    x, kw, _, _ = _inputs(gauss, pool, rows, 2, 2, True, S)
    plain = {k: v for k, v in kw.items() if k not in ("sigma", "peer_sigma")}
    for route in ("staged", "global"):
        want = gauss.stored[pool[0]].predict_quantiles(x, PROBS, route=route, **plain)
        got = gauss.stored[pool[0]].predict_ppd(x, PROBS, row_scale=np.zeros(rows), noise_key=KEY, route=route, **kw)
        assert np.array_equal(got["quantiles"], want["quantiles"]), f"S {S} {route}: not predict_quantiles' bits"
        same = ("route", "rows_per_chunk", "chunks", "rows_per_sort", "padded_draws", "largest_draw_nodes", "launches", "draws")
        assert all(got["info"][k] == want["info"][k] for k in same) and all(got[k] is None for k in SCORES)


@pytest.mark.parametrize("rows", [127, 128, 129])
def test_rows_around_a_workgroup(gauss, rows):
    got, *_ = _case(gauss, POOLS[18], rows, f"{rows} rows, 128 per workgroup", M=1, seed=rows)
    assert got["info"]["rows_per_sort"] == 128 and got["info"]["padded_draws"] == 32


@pytest.mark.parametrize("times,rows", [(316, 70), (1260, 3)])
def test_one_row_per_workgroup_up_to_the_lds_maximum(gauss, times, rows):
    """4 108 draws: one row per workgroup, all four waves on it; 16 380 draws: 128 KB of keys.  A handle pooled repeatedly, each with the same sigma."""
    S = 13 * times
    x = np.asfortranarray(gauss.x[:rows])
    probs = (0.0, 0.025, 0.5, 0.975, 1.0)
    sg = _sigma(13, 0, times)
    bart = gauss.bart(13)[:rows]
    y, rs = bart.mean(axis=1) + np.random.default_rng(times).standard_normal(rows), _row_scale(rows, times)
    got = gauss.stored[13].predict_ppd(x, probs, y=y, sigma=sg, row_scale=rs, noise_key=KEY, peers=[gauss.stored[13]] * (times - 1), peer_sigma=[sg] * (times - 1))
    sp = 1 << (S - 1).bit_length()
    assert got["draws"] == S and got["info"]["padded_draws"] == sp and got["info"]["rows_per_sort"] == 1 and sp == (8192 if times == 316 else 16384)
    z = np.tile(bart, (1, times))
    ref, bd = pp.from_z(z, np.zeros_like(z), np.tile(sg, times), KEY, probs, y=y, row_scale=rs)
    pp.assert_ppd(got, ref, bd, f"S {S}", _report)


def test_chunks_live_and_stored_samplers_determinism_and_the_key(gauss):
    pool, S, rows = POOLS[18], 18, 1037
    whole, (x, kw), _ = _case(gauss, pool, rows, f"{rows} rows in one chunk", M=1, E=1, offset=True, seed=4)
    assert whole["info"]["chunks"] == 1 and whole["info"]["rows_per_chunk"] == rows and whole["info"]["launches"] == 2
    smp = gauss.stored[pool[0]]
    for C, chunks in ((64, 17), (192, 6)):
        for route in ("staged", "global"):
            got = smp.predict_ppd(x, PROBS, scratch_bytes=8 * S * C + 8 * S * 63, route=route, **kw)          # (rounded down to 64 rows)
            info = got["info"]
            assert (info["rows_per_chunk"], info["chunks"], info["launches"]) == (C, chunks, 2 * chunks), info
            assert rows - (chunks - 1) * C in (13, 77)
            _same_bits(got, whole, f"{rows} rows in chunks of {C}, {route}")
    per_row = ("offset", "dense", "ell_index", "ell_value", "y", "row_scale")
    few = {k: (v[:130] if k in per_row else v) for k, v in kw.items()}
    tiny = smp.predict_ppd(x[:130], PROBS, scratch_bytes=1, **few)
    assert tiny["info"]["rows_per_chunk"] == 64 and tiny["info"]["chunks"] == 3          # at least 64 rows per chunk
    _same_bits(tiny, {k: (whole[k][..., :130] if whole[k] is not None else None) for k in ("quantiles",) + SCORES}, "scratch_bytes 1")
    # the same call twice; the live sampler holds the kept trees of stored[13]: as a peer and, with the tables swapped, not compared (the pool's order moves the noise)
    _same_bits(smp.predict_ppd(x, PROBS, **kw), whole, "the same call twice")
    live = smp.predict_ppd(x, PROBS, **dict(kw, peers=[gauss.live]))
    _same_bits(live, whole, "a live sampler as the peer")
    own13 = {k: v for k, v in kw.items() if k not in ("peers", "peer_sigma", "peer_dense_coef", "peer_ell_coef")}
    own13.update(sigma=kw["peer_sigma"][0], dense_coef=kw["peer_dense_coef"][0], ell_coef=kw["peer_ell_coef"][0])
    _same_bits(gauss.live.predict_ppd(x, PROBS, **own13), gauss.stored[13].predict_ppd(x, PROBS, **own13), "live and stored sampler as the caller")
    # another key: other noise, the same scores
    other = smp.predict_ppd(x, PROBS, **dict(kw, noise_key=KEY + 1))
    _same_bits(other, whole, "another noise key", SCORES)
    assert not np.array_equal(other["quantiles"], whole["quantiles"]) and np.mean(other["quantiles"] != whole["quantiles"]) > 0.99


def test_device_memory_of_a_call(gauss):
    S, rows = 13, 700
    got, *_ = _case(gauss, (S,), rows, "device memory", M=2, E=2, offset=True, seed=S, scratch_bytes=8 * S * 192)
    nodes = struct.unpack_from("<Q", gauss.stored[S].export_bart_state(), 28)[0]
    want = pp.device_bytes_formula(gauss.P, rows, nodes, S, gauss.T, True, 2, 2, 7, 192, len(PROBS), 0, True, True, True, True, True)
    assert got["info"]["rows_per_chunk"] == 192 and got["info"]["device_bytes"] == want, (got["info"], want)


def test_binary_response(gauss, binary):
    """Link 1: l = log Phi(+-z).  The offset plants z from one end of [-8, 8] to the other, y alternates: rows whose response is all but impossible
    under every draw (l below -12) beside rows it is all but certain for."""
    assert binary.args.is_binary
    rows = 300
    for pool in (POOLS[18], POOLS[5]):
        x = np.asfortranarray(binary.x[:rows])
        bart = np.concatenate([binary.bart(S)[:rows] for S in pool], axis=1)
        spread = float(np.abs(bart - bart.mean(axis=1, keepdims=True)).max())
        tmax = 8.0 - spread - 0.01
        assert tmax > 5.0, spread
        off = np.linspace(-tmax, tmax, rows) - bart.mean(axis=1)
        y = (np.arange(rows) % 2).astype(np.float64)
        parts = [dict(bart=binary.bart(S)[:rows]) for S in pool]
        ref, bd = pp.model(parts, y=y, link=1, offset=off)
        assert np.abs(ref["z"]).max() > 5.0 and ref["l"].min() < -12.0 and ref["l"].max() > -1e-6 and "pit" not in ref
        res = {}
        for route in ("staged", "global"):
            res[route] = binary.stored[pool[0]].predict_ppd(x, (), y=y, offset=off, link=1, peers=[binary.stored[S] for S in pool[1:]], route=route)
            pp.assert_ppd(res[route], ref, bd, f"binary response, {sum(pool)} draws, {route}", _report)
        _same_bits(res["staged"], res["global"], "link 1: the two routes")
    smp, before = binary.stored[5], binary.live.get_counters()
    for match, kw in (("pit must be NULL under link 1", dict(pit=True)), ("n_probs > 0 under link 1: no y_rep is formed", dict(probs=(0.5,))),
                      ("under link 1 every y is 0 or 1", dict(y=np.where(np.arange(rows) == 17, 0.5, y)))):
        with pytest.raises(RuntimeError, match=match):
            smp.predict_ppd(x, **{"probs": (), "y": y, "offset": off, "link": 1, **kw})
        assert not any(smp.ppd_info.values())
    assert np.array_equal(binary.live.get_counters(), before)


def test_score_extremes(gauss):
    """Link 0 with sigma far below the spread of the draws: a response equal to one draw's z (that draw dominates the sum), one at the row's mean and
    one 40 sd beyond every draw (l near -800: exp(l) is 0 in double, the shift by the maximum carries the sum)."""
    rows, S = 300, 13
    x = np.asfortranarray(gauss.x[:rows])
    z = gauss.bart(S)[:rows]
    sg = np.full(S, 1e-3 * float(z.std()))
    kind = np.arange(rows) % 3
    y = np.where(kind == 0, z[:, 3], np.where(kind == 1, z.mean(axis=1), z.max(axis=1) + 40.0 * sg[0]))
    ref, bd = pp.from_z(z, np.zeros_like(z), sg, y=y)
    far = ref["l"][kind == 2]
    assert far.max() < -780.0 and far.min() > -1e9 and np.exp(far.max()) == 0.0
    top2 = np.sort(ref["l"][kind == 0], axis=1)[:, -2:]
    assert np.median(top2[:, 1] - top2[:, 0]) > 30.0, "no draw dominates the sum"
    got = gauss.stored[S].predict_ppd(x, (), y=y, sigma=sg)
    pp.assert_ppd(got, ref, bd, "score extremes", _report)
    assert np.all(np.isfinite(got["lpd"])) and np.all(got["pit"][kind == 2] == 1.0)
    # one draw: lm2 = 0 and lpd = l
    z1 = gauss.bart(1)[:rows]
    y1 = z1[:, 0] + np.linspace(-3.0, 3.0, rows)
    ref1, bd1 = pp.from_z(z1, np.zeros_like(z1), [0.7], y=y1)
    one = gauss.stored[1].predict_ppd(x, (), y=y1, sigma=[0.7])
    pp.assert_ppd(one, ref1, bd1, "one draw", _report)
    assert np.array_equal(one["lm2"], np.zeros(rows)) and np.array_equal(one["lpd"], one["lmean"])


def test_refusals_come_before_any_launch(hip_lib, gauss, binary):
    from conftest import make_sampler
    rows, S = 50, 13
    x = np.asfortranarray(gauss.x[:rows])
    live = gauss.live
    y, sg = np.zeros(rows), np.ones(S)
    parts = sc.linear_parts(rows, S, 1, 2)
    peer = sc.linear_parts(rows, 5, 1, 2, seed=1)

    def bad(a, at, v):
        a = np.array(a, dtype=np.float64)
        a[at] = v
        return a

    def refused(match, probs=(0.5,), samplers=None, **kw):
        before = live.get_counters()
        for smp in samplers or (live, gauss.stored[S]):
            with pytest.raises(RuntimeError, match=match):
                smp.predict_ppd(x, probs, **{"sigma": sg, **kw})
            assert smp.ppd_info["launches"] == 0 and not any(smp.ppd_info.values())
        assert np.array_equal(live.get_counters(), before), "a refused call launched something"
    for v in (0.0, -1.0, np.nan, np.inf):
        refused(r"sigma holds \S+ at draw 4 \(every sigma must be finite and > 0\)", sigma=bad(sg, 4, v))
        refused(r"peer_sigma\[0\] holds \S+ at draw 2", peers=[gauss.stored[5]], peer_sigma=[bad(np.ones(5), 2, v)])
    refused("link 0 needs sigma", sigma=None)
    refused("link 0 needs peer_sigma", peers=[gauss.stored[5]])
    for v in (-0.5, np.nan, np.inf):
        refused(r"row_scale holds \S+ at row 7 \(finite and >= 0\)", row_scale=bad(np.ones(rows), 7, v))
    refused("row_scale is 0 at row 7: with y every row_scale must be > 0", y=y, row_scale=bad(np.ones(rows), 7, 0.0))
    for v in (np.nan, np.inf, -np.inf):
        refused(r"y holds \S+ at row 9 \(every y must be finite\)", y=bad(y, 9, v))
    refused("under link 1 every y is 0 or 1", probs=(), y=bad(y, 9, 2.0), link=1, sigma=None, samplers=(binary.stored[5],))
    refused("nothing asked for", probs=())
    refused("nothing asked for", probs=(), y=y, lpd=False, moments=False, pit=False)
    refused("between 0 and 16 probs per call, not 17", probs=np.linspace(0, 1, 17))
    refused(r"prob 1\.5\d* outside \[0, 1\]", probs=(1.5,))
    refused(r"prob -?nan outside \[0, 1\]", probs=(0.1, np.nan))
    refused("link must be 0", link=2)
    refused("negative scratch_bytes", scratch_bytes=-1)
    # lmean without lm2 (the Python method gives both or neither: the structure is filled here)
    import ctypes as C
    from stan4bart_amd.abi import PpdIn, PpdOut, Sampler
    rows_in, keep, _, _ = Sampler._summary_in(S, x, None, None, None, None, None, None, 0, None, "auto", 0, 0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))          # noqa: E731
    buf = np.zeros(rows)
    arg = PpdIn(rows=rows_in, y=dp(y), sigma=dp(sg))
    before = live.get_counters()
    for out in (PpdOut(lmean=dp(buf)), PpdOut(lm2=dp(buf))):
        assert hip_lib.s4b_predict_ppd(live._h, C.byref(arg), C.byref(out)) == 1
        assert "lmean and lm2 are given together or not at all" in hip_lib.s4b_last_error().decode() and not any(out.info)
    out = PpdOut(lpd=dp(buf))
    arg.y = None
    assert hip_lib.s4b_predict_ppd(live._h, C.byref(arg), C.byref(out)) == 1 and "need y" in hip_lib.s4b_last_error().decode() and not any(out.info)
    assert np.array_equal(live.get_counters(), before)
    # the pool: 16 393 draws, and every peer rule of predict_quantiles
    with pytest.raises(RuntimeError, match="16393 pooled draws, at most 16384"):
        live.predict_ppd(x[:3], [0.5], sigma=sg, peers=[gauss.stored[13]] * 1260, peer_sigma=[sg] * 1260)
    assert not any(live.ppd_info.values())
    assert binary.args.n_trees != gauss.args.n_trees
    refused("peer 1 has 11 trees per draw, the sampler 25", peers=[gauss.stored[5], binary.stored[5]], peer_sigma=[np.ones(5)] * 2)
    refused("peer 0 has a binary response, the sampler a continuous one|peer 0 has 11 trees", peers=[binary.stored[5]], peer_sigma=[np.ones(5)])
    refused("n_dense > 0 needs peer_dense_coef", peers=[gauss.stored[5]], peer_sigma=[np.ones(5)], dense=parts["dense"], dense_coef=parts["dense_coef"])
    refused("n_ell > 0 needs peer_ell_coef", peers=[gauss.stored[5]], peer_sigma=[np.ones(5)], peer_dense_coef=[peer["dense_coef"]], **parts)
    other = make_sampler(hip_lib, "s4b_", rc._friedman(n=410, T=25, warmup=2, iter=3, ranef=False))          # trained on other rows: other cut points
    fresh = make_sampler(hip_lib, "s4b_", gauss.args)          # keep_trees, but no sampling run yet
    try:
        other.run(2, True)
        other.disengage_adaptation()
        other.run(1, False)
        refused(r"peer 0 has other cut points of predictor \d+", peers=[other], peer_sigma=[np.ones(1)])
        refused("peer 1 holds no kept draws", peers=[gauss.stored[5], fresh], peer_sigma=[np.ones(5), np.ones(0)])
        refused("the sampler holds no kept draws", samplers=(fresh,), sigma=np.ones(0))
    finally:
        other.free()
        fresh.free()
    before = live.get_counters()
    ok = live.predict_ppd(x, [0.5], y=y, sigma=sg, peers=[gauss.stored[5]], peer_sigma=[np.ones(5)], peer_dense_coef=[peer["dense_coef"]],
                          peer_ell_coef=[peer["ell_coef"]], **parts)
    assert ok["info"]["launches"] == 2 and live.get_counters()[2] == before[2] + 2 and ok["draws"] == 18
    del keep


def test_whole_interface(hip_lib):
    """Stan4bartFit.predict_ppd against fit.predict(type="ev") and extract("sigma") put through the numpy model with the returned noise_key: two
    chains, fixed effects, random intercepts, a continuous response, observation weights; coverage and elpd_waic_total recomputed from the matrix."""
    from stan4bart_amd import GroupTerm, generate_friedman_data
    from stan4bart_amd.abi import Sampler
    from stan4bart_amd.generics import combine_chains_f, stan4bart
    d = generate_friedman_data(120, ranef=True, causal=True, p=10)
    x = d["x"]
    xb, X = x[:, [j for j in range(10) if j != 3]], np.column_stack([x[:, 3], d["z"]])
    groups = [GroupTerm(d["g1"], None, "g.1"), GroupTerm(d["g2"], None, "g.2")]
    fit = stan4bart(d["y"], xb, X=X, groups=groups, chains=2, seed=99, iter=14, warmup=6, bart_args={"n.trees": 9, "keepTrees": True},
                    make_sampler=lambda a, st: Sampler(hip_lib, "s4b_", a, st))
    try:
        m = 45
        g = np.random.default_rng(3)
        new = [GroupTerm(np.asarray(d["g1"])[:m], None, "g.1"), GroupTerm(np.asarray(d["g2"])[:m], None, "g.2")]
        xb_new, X_new = xb[:m] + 0.01 * g.normal(size=(m, 9)), X[:m] + 0.05 * g.normal(size=(m, 2))
        y_new = np.asarray(d["y"], dtype=np.float64)[:m] + 0.5 * g.normal(size=m)          # stand-ins for held-out responses near the training ones
        w = g.uniform(0.5, 2.0, m)
        full = fit.predict(x_bart=xb_new, X=X_new, groups=new, type="ev", combine_chains=False, seed=7)          # [rows, iter, chain]
        assert full.shape == (m, 8, 2)
        flat, sigma = combine_chains_f(full), fit.extract("sigma")
        assert sigma.shape == (16,) and np.all(sigma > 0)
        # the bound of a value: the model over the builder's own tables, once for the device and once more for the arithmetic of fit.predict itself
        ix, val, coef = fit._ell_random(new, True, np.random.default_rng(7))
        beta = fit.stan[fit._rows("beta.")]
        bart = np.concatenate([s.predict_bart(xb_new) for s in fit.samplers], axis=1)
        mref, mbound = sc.model(bart, None, X_new - fit.X_means, np.concatenate([beta[:, :, c].T for c in range(2)]), ix, val, np.concatenate(coef))
        assert sc.bound_ratio(flat, mref["v"], mbound["v"]) <= sc.BOUND_FACTOR, "fit.predict and the model over the ELL table describe different draws"
        probs = (0.05, 0.5, 0.95)
        got = fit.predict_ppd(xb_new, X=X_new, groups=new, y=y_new, probs=probs, obs_weights=w, seed=7)
        assert got["draws"] == 16 and got["quantiles"].shape == (3, m) and np.array_equal(got["probs"], probs) and got["seed"] == 7
        ref, bd = pp.from_z(flat, 2.0 * np.broadcast_to(mbound["v"], flat.shape), sigma, got["noise_key"], probs, y=y_new, row_scale=1.0 / np.sqrt(w))
        for key in ("quantiles", "lpd", "pit"):
            r = pp.bound_ratio(got[key], ref[key], bd[key])
            print(f"whole interface: {key}, max |device - model over fit.predict| / bound = {r:.3g}")
            assert r <= pp.BOUND_FACTOR, (key, r)
        p_waic = ref["lm2"] / 15
        assert pp.bound_ratio(got["p_waic"], p_waic, bd["lm2"] / 15 + pp.U * p_waic) <= pp.BOUND_FACTOR
        elpd = ref["lpd"] - p_waic
        assert abs(got["elpd_waic_total"] - elpd.sum()) <= pp.BOUND_FACTOR * float((bd["lpd"] + bd["lm2"] / 15 + 2 * pp.U * np.abs(elpd)).sum() + m * pp.U * np.abs(elpd).sum())
        assert got["se"] == pytest.approx(np.sqrt(m * np.var(elpd, ddof=1)), rel=1e-9)
        inside = (y_new >= ref["quantiles"][0]) & (y_new <= ref["quantiles"][2])
        assert got["coverage"] == inside.mean() and 0.3 < got["coverage"] <= 1.0
        # the same seed: the same bits; the returned key alone does not move the scores
        again = fit.predict_ppd(xb_new, X=X_new, groups=new, y=y_new, probs=probs, obs_weights=w, seed=7)
        assert again["noise_key"] == got["noise_key"] and np.array_equal(again["quantiles"], got["quantiles"]) and np.array_equal(again["lpd"], got["lpd"])
    finally:
        fit.close()
