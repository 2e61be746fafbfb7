"""s4b_predict_loo on the device (stan4bart_amd/csrc/dev_loo.inc: k_predict_values<staged / global> unchanged, k_loo_rows) against numpy on the full
pooled matrix (tests/loo_cases.py: the model, the bound, the rows left out).  Pool sizes 1, 2, 20 (no fit), 21 (the first fit), 5 + 13 with a sigma
vector per peer, 64 / 65, 1024 / 1025 / 2048 / 2049 (one, two, four waves per row), 4108 and 16380 (one row per workgroup, the LDS maximum), a given
tail of 5 and of 1024; rows around a workgroup, chunks, both routes, live and stored samplers, determinism; planted rows (a constant likelihood, a
response 40 sd out, tail values tied with the cutoff, a tail that underflows); a binary response; the refusals before any launch; the device bytes;
lpd against predict_ppd's; the whole Python interface.

One small Friedman chain per response kind, as tests/test_gpu_predict_ppd.py builds them: stored samplers of 1, 2, 5 and 13 draws, pooled repeatedly —
each occurrence with a sigma vector of its own, so that the repeated draws do not tie — for the larger pools."""
import struct

import numpy as np
import pytest

import loo_cases as lc
import pd_cases as pc
import ppd_cases as pp
import readout_cases as rc
import summary_cases as sc

pytestmark = pytest.mark.gpu
POOLS = {1: (1,), 2: (2,), 18: (5, 13), 20: (13, 5, 2), 21: (13, 5, 2, 1), 64: (13,) * 4 + (5, 5, 2), 65: (13,) * 5,
         1024: (13,) * 78 + (5, 5), 1025: (13,) * 78 + (5, 5, 1), 2048: (13,) * 157 + (5, 2), 2049: (13,) * 157 + (5, 2, 1),
         4108: (13,) * 316, 5200: (13,) * 400, 16380: (13,) * 1260}
assert all(sum(v) == k for k, v in POOLS.items())
WORST = {}


def _report(line):
    print(line)


def _note(ratios):
    for k, r in ratios.items():
        WORST[k] = max(WORST.get(k, 0.0), r)


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
    print("predict_loo, largest |device - model| / bound of this module: " + ", ".join(f"{k} {r:.3g}" for k, r in WORST.items()))


@pytest.fixture(scope="module")
def binary(hip_lib):
    c = Chain(hip_lib, rc._binary(n=400, T=11, warmup=6, iter=19), rows=400)
    yield c
    c.close()


def _sigma(S, j, seed):
    return np.random.default_rng([9100, seed, j, S]).uniform(0.5, 2.0, S)


def _inputs(chain, pool, rows, M=0, E=0, offset=False, seed=0):
    """The arguments of a pooled call over the first `rows` rows and the model's `parts` (tests/test_gpu_predict_ppd.py's): the row side is shared,
    every pooled sampler — every OCCURRENCE of a handle — gets coefficient tables and a sigma vector of its own."""
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


def _responses(z, sd_row, seed):
    """Responses around the rows' predictions: three quarters within about one sd, one quarter 2 to 4 sd out (the heavy-tail regime)."""
    g = np.random.default_rng([7100, seed])
    rows = len(z)
    far = g.uniform(size=rows) < 0.25
    t = np.where(far, g.uniform(2.0, 4.0, rows) * g.choice([-1.0, 1.0], rows), g.standard_normal(rows))
    return z.mean(axis=1) + (z.std(axis=1) + sd_row) * t


def _row_scale(z, seed):
    """Row scales between half and six times the spread of the row's own draws: with sigma in [0.5, 2] the likelihoods of a row stay within a few
    hundred of each other, so no importance ratio underflows against the largest (long double and double underflow at different arguments; the
    planted rows carry that case)."""
    return np.random.default_rng([8100, seed]).uniform(0.25, 3.0, len(z)) * 2.0 * np.maximum(z.std(axis=1), 0.1)


_REF = {}


def _case(chain, pool, rows, what, M=0, E=0, offset=False, seed=0, tail=0, **call):
    """One pooled call against the model; the reference of a case is computed once and shared by the routes."""
    x, kw, parts, row_side = _inputs(chain, pool, rows, M, E, offset, seed)
    ck = (id(chain), pool, rows, M, E, offset, seed, tail)
    if ck not in _REF:
        z, _ = pp.pooled_z(parts, **row_side)
        rs = _row_scale(z, seed)
        y = _responses(z, 1.2 * rs, seed)
        _REF[ck] = (y, rs) + lc.model(parts, y, tail or None, row_scale=rs, what=what, **row_side)
    y, rs, ref, bd, compared = _REF[ck]
    got = chain.stored[pool[0]].predict_loo(x, y=y, row_scale=rs, tail_len=tail, **kw, **call)
    S = sum(pool)
    assert got["draws"] == S and got["info"]["draws"] == S and got["info"]["launches"] == 2 * got["info"]["chunks"]
    assert got["tail_len"] == (tail or lc.tail_len(S))
    _note(lc.assert_loo(got, ref, bd, compared, what, _report))
    return got, (x, dict(kw, y=y, row_scale=rs, tail_len=tail)), (ref, bd, compared)


def _same_bits(a, b, what, keys=lc.OUTPUTS):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            assert np.array_equal(a[k], b[k]), f"{what}: {k} differs"


@pytest.mark.parametrize("S", [1, 2, 18, 20, 21, 64, 65])
def test_small_pools_against_the_model_on_both_routes(gauss, S):
    pool, rows = POOLS[S], 300
    res = {}
    for route in ("staged", "global"):
        res[route], _, (ref, bd, compared) = _case(gauss, pool, rows, f"S {S} {route}", M=2, E=2, offset=True, seed=S, route=route)
        info = res[route]["info"]
        sp = 1 << (S - 1).bit_length()
        assert info["route"] == (1 if route == "staged" else 2) and info["padded_draws"] == sp and info["rows_per_sort"] == 4096 // sp
        assert info["rows_per_chunk"] == rows and info["chunks"] == 1
    _same_bits(res["staged"], res["global"], f"S {S}: the two routes")
    got = res["staged"]
    if S <= 20:          # M < 5: no fit anywhere
        assert got["tail_len"] < 5 and np.all(np.isposinf(got["pareto_k"]))
    else:
        assert got["tail_len"] >= 5 and np.isfinite(got["pareto_k"]).mean() > 0.9, "the fit is not reached"
    assert np.all(got["ess"] >= 1.0 - 1e-12) and np.all(got["ess"] <= S * (1.0 + 1e-12)) and np.all(got["elpd_loo"] <= got["lpd"] + 1e-9)
    if S == 1:
        assert np.array_equal(got["ess"], np.ones(rows)) and np.array_equal(got["elpd_loo"], got["lpd"])
    if S == 18:          # every peer's own sigma reached its draws: the model with the first table for all is another answer
        x, kw, parts, row_side = _inputs(gauss, pool, rows, 2, 2, True, S)
        same = [dict(p, sigma=np.resize(parts[0]["sigma"], len(p["sigma"]))) for p in parts]
        y, rs = _REF[(id(gauss), pool, rows, 2, 2, True, S, 0)][:2]
        other, obd, _ = lc.model(same, y, row_scale=rs, **row_side)
        assert lc.bound_ratio(got["elpd_loo"], other["elpd_loo"], obd["elpd_loo"]) > 1e6, "the peers' sigma vectors do not matter: the case tests no per-peer sigma"


def _repeated(chain, pool, rows, seed, tail=0):
    """A pool of many occurrences of few handles, no linear part: z is the stored samplers' predict_bart, known exactly."""
    x = np.asfortranarray(chain.x[:rows])
    sigmas = [_sigma(S, j, seed) for j, S in enumerate(pool)]
    z = np.concatenate([chain.bart(S)[:rows] for S in pool], axis=1)
    rs = _row_scale(z, seed)
    y = _responses(z, 1.2 * rs, seed)
    kw = dict(y=y, sigma=sigmas[0], row_scale=rs, peers=[chain.stored[S] for S in pool[1:]], peer_sigma=sigmas[1:], tail_len=tail)
    ref, bd, compared = lc.from_z(z, np.zeros_like(z), np.concatenate(sigmas), y, tail or None, rs, what=f"S {sum(pool)}")
    return x, kw, (ref, bd, compared)


@pytest.mark.parametrize("S,per_sort", [(1024, 4), (1025, 2), (2048, 2), (2049, 1)])
def test_one_two_and_four_waves_per_row(gauss, S, per_sort):
    rows = 50
    x, kw, (ref, bd, compared) = _repeated(gauss, POOLS[S], rows, S)
    got = gauss.stored[POOLS[S][0]].predict_loo(x, **kw)
    assert got["draws"] == S and got["info"]["rows_per_sort"] == per_sort and got["info"]["padded_draws"] == 1 << (S - 1).bit_length()
    assert got["tail_len"] == lc.tail_len(S) and np.isfinite(got["pareto_k"]).all()
    _note(lc.assert_loo(got, ref, bd, compared, f"S {S}", _report))


@pytest.mark.parametrize("S,rows,tail,grid", [(4108, 24, 193, 43), (16380, 6, 384, 49)])
def test_one_row_per_workgroup_up_to_the_lds_maximum(gauss, S, rows, tail, grid):
    x, kw, (ref, bd, compared) = _repeated(gauss, POOLS[S], rows, S)
    got = gauss.stored[13].predict_loo(x, **kw)
    sp = 1 << (S - 1).bit_length()
    assert got["draws"] == S and got["info"]["padded_draws"] == sp and got["info"]["rows_per_sort"] == 1 and sp == (8192 if S == 4108 else 16384)
    assert got["tail_len"] == tail == lc.tail_len(S) and 30 + int(np.sqrt(tail)) == grid
    _note(lc.assert_loo(got, ref, bd, compared, f"S {S}", _report))


@pytest.mark.parametrize("tail", [5, 1024])
def test_a_given_tail_length(gauss, tail):
    S, rows = 5200, 8
    x, kw, (ref, bd, compared) = _repeated(gauss, POOLS[S], rows, S + tail, tail=tail)
    got = gauss.stored[13].predict_loo(x, **kw)
    assert got["tail_len"] == tail and got["info"]["padded_draws"] == 8192 and lc.lds_bytes(S, tail) == 65536 + 256 + 8 * tail
    _note(lc.assert_loo(got, ref, bd, compared, f"S {S}, tail {tail}", _report))
    if tail == 5:
        assert not np.array_equal(got["elpd_loo"], gauss.stored[13].predict_loo(x, **dict(kw, tail_len=0))["elpd_loo"])


@pytest.mark.parametrize("rows", [127, 128, 129])
def test_rows_around_a_workgroup(gauss, rows):
    got, *_ = _case(gauss, POOLS[21], rows, f"{rows} rows, 128 per workgroup", M=1, seed=rows)
    assert got["info"]["rows_per_sort"] == 128 and got["info"]["padded_draws"] == 32


def test_chunks_live_and_stored_samplers_and_determinism(gauss):
    pool, S, rows = POOLS[21], 21, 1037
    whole, (x, kw), _ = _case(gauss, pool, rows, f"{rows} rows in one chunk", M=1, E=1, offset=True, seed=4)
    assert whole["info"]["chunks"] == 1 and whole["info"]["rows_per_chunk"] == rows and whole["info"]["launches"] == 2
    smp = gauss.stored[pool[0]]
    for C, chunks in ((64, 17), (192, 6)):
        for route in ("staged", "global"):
            got = smp.predict_loo(x, scratch_bytes=8 * S * C + 8 * S * 63, route=route, **kw)          # (rounded down to 64 rows)
            info = got["info"]
            assert (info["rows_per_chunk"], info["chunks"], info["launches"]) == (C, chunks, 2 * chunks), info
            assert rows - (chunks - 1) * C in (13, 77)
            _same_bits(got, whole, f"{rows} rows in chunks of {C}, {route}")
    per_row = ("offset", "dense", "ell_index", "ell_value", "y", "row_scale")
    few = {k: (v[:130] if k in per_row else v) for k, v in kw.items()}
    tiny = smp.predict_loo(x[:130], scratch_bytes=1, **few)
    assert tiny["info"]["rows_per_chunk"] == 64 and tiny["info"]["chunks"] == 3          # at least 64 rows per chunk
    _same_bits(tiny, {k: whole[k][:130] for k in lc.OUTPUTS}, "scratch_bytes 1")
    _same_bits(smp.predict_loo(x, **kw), whole, "the same call twice")
    # the live sampler holds the kept trees of stored[13]: as the caller it returns the stored sampler's bits
    _same_bits(gauss.live.predict_loo(x, **kw), whole, "live and stored sampler as the caller")
    swapped = dict(kw, peers=[gauss.live if p is gauss.stored[13] else p for p in kw["peers"]])
    _same_bits(smp.predict_loo(x, **swapped), whole, "the same peers")
    # only the outputs asked for are formed, with the same bits
    part = smp.predict_loo(x, outputs=("pareto_k", "ess"), **kw)
    assert part["elpd_loo"] is None and part["lpd"] is None
    _same_bits(part, whole, "two outputs of four", ("pareto_k", "ess"))


def test_device_memory_of_a_call(gauss):
    pool, rows = POOLS[21], 700
    got, *_ = _case(gauss, pool, rows, "device memory", M=2, E=2, offset=True, seed=21, scratch_bytes=8 * 21 * 192)
    nodes = sum(struct.unpack_from("<Q", gauss.stored[S].export_bart_state(), 28)[0] for S in pool)
    want = lc.device_bytes_formula(gauss.P, rows, nodes, 21, gauss.T, True, 2, 2, 7, 192, 0, True, 4)
    assert got["info"]["rows_per_chunk"] == 192 and got["info"]["device_bytes"] == want, (got["info"], want)


def test_planted_rows_take_their_branch_per_row(gauss):
    """Pool 13 + 13 of one handle with ONE sigma for every draw and a tail of 7: every likelihood occurs twice, so sorted positions 18 (the cutoff)
    and 19 (the first of the tail) tie and x_0 = 0 in every row.  Beside the ordinary rows, two of each: a constant likelihood (an ELL column holds
    -bart of the row: z = bart - bart = 0 for every draw; the tail is equal: +inf), a response 40 sd beyond every draw with sd the spread of the row's
    draws (l near -800, one draw dominating, khat > 1), and a response AT one draw under a row scale of 1e-3 (the other draws' ratios underflow against
    the largest: exp(lw) = 0 below the cutoff and over most of the tail; long double and double underflow at different arguments, so the model may
    leave these rows out — the device must still return finite results there)."""
    rows, S, M = 300, 26, 7
    x = np.asfortranarray(gauss.x[:rows])
    bart = gauss.bart(13)[:rows]
    z = np.concatenate([bart, bart], axis=1)
    const, far, under = (7, 207), (19, 219), (33, 233)
    ell_index = np.full((rows, 1), -1, dtype=np.int32)
    ell_coef = np.zeros((13, 2))
    for c, i in enumerate(const):
        ell_index[i, 0] = c
        ell_coef[:, c] = -bart[i]
        z[i] = 0.0
    spread = float(bart.std())
    sg = np.full(13, 0.8 * spread)
    rs = np.full(rows, 1.0)
    rs[list(under)] = 1e-3
    for i in far:
        rs[i] = z[i].std() / sg[0]          # sd = the spread of the row's own draws: their likelihoods stay within a few hundred of each other
    y = _responses(z, sg[0] * rs, 26)
    y[list(const)] = 0.3
    for i in far:
        y[i] = z[i].max() + 40.0 * sg[0] * rs[i]
    for i in under:
        y[i] = z[i, 3]
    ref, bd, compared = lc.from_z(z, np.zeros_like(z), np.concatenate([sg, sg]), y, M, rs, what="planted rows")
    srt = np.sort(-ref["l"], axis=1)
    assert np.all(srt[:, S - M] == srt[:, S - M - 1]), "the first tail value does not tie with the cutoff"
    assert np.all(ref["l"][list(far)].max(axis=1) < -780.0) and np.all(np.isfinite(ref["pareto_k"][list(far)])) and np.all(ref["pareto_k"][list(far)] > 1.0)
    assert np.all(np.exp(srt[list(under), S - M - 1] - srt[list(under), -1]) == 0.0), "the cutoff of the underflow rows does not underflow"
    assert np.all(np.isposinf(ref["pareto_k"][list(const)]))
    got = gauss.stored[13].predict_loo(x, y=y, sigma=sg, row_scale=rs, tail_len=M, peers=[gauss.stored[13]], peer_sigma=[sg], ell_index=ell_index,
                                       ell_value=np.ones((rows, 1)), ell_coef=ell_coef, peer_ell_coef=[ell_coef])
    assert got["info"]["rows_per_sort"] == 128
    _note(lc.assert_loo(got, ref, bd, compared, "planted rows", _report))
    lconst = -pp.C_HALF_LOG_2PI - np.log(sg[0]) - 0.5 * (0.3 / sg[0]) ** 2
    for i in const:
        assert np.isposinf(got["pareto_k"][i]) and abs(got["elpd_loo"][i] - lconst) <= 1e-13 and abs(got["ess"][i] - S) <= 1e-10, (i, got["elpd_loo"][i], lconst)
    assert np.all(got["pareto_k"][list(far)] > 1.0) and np.all(np.isfinite(got["pareto_k"][list(far)]))
    ordinary = np.setdiff1d(np.arange(rows), const + far + under)
    assert np.isfinite(got["pareto_k"][ordinary]).mean() > 0.95, "the planted rows changed the branch of their neighbours"


def test_binary_response(binary):
    """Link 1: l = log Phi(+-z).  The offset plants z from one end of [-8, 8] to the other, y alternates (tests/test_gpu_predict_ppd.py's case).  One
    sampler of 13 draws with a given tail of 5: the stored samplers of a chain are nested, and without a sigma to tell the occurrences apart a pool of
    them would tie most of its likelihoods."""
    assert binary.args.is_binary
    rows, S, M = 300, 13, 5
    x = np.asfortranarray(binary.x[:rows])
    bart = binary.bart(S)[:rows]
    spread = float(np.abs(bart - bart.mean(axis=1, keepdims=True)).max())
    tmax = 8.0 - spread - 0.01
    assert tmax > 5.0, spread
    off = np.linspace(-tmax, tmax, rows) - bart.mean(axis=1)
    y = (np.arange(rows) % 2).astype(np.float64)
    ref, bd, compared = lc.model([dict(bart=bart)], y, M, link=1, offset=off, what="binary response")
    assert ref["l"].min() < -12.0 and ref["l"].max() > -1e-6 and np.isfinite(ref["pareto_k"]).mean() > 0.9
    res = {}
    for route in ("staged", "global"):
        res[route] = binary.stored[S].predict_loo(x, y=y, offset=off, link=1, tail_len=M, route=route)
        _note(lc.assert_loo(res[route], ref, bd, compared, f"binary response, {S} draws, {route}", _report))
    _same_bits(res["staged"], res["global"], "link 1: the two routes")
    _same_bits(binary.live.predict_loo(x, y=y, offset=off, link=1, tail_len=M), res["staged"], "link 1: the live sampler")
    with pytest.raises(RuntimeError, match="under link 1 every y is 0 or 1"):
        binary.stored[13].predict_loo(x, y=np.where(np.arange(rows) == 17, 0.5, y), offset=off, link=1)
    assert not any(binary.stored[13].loo_info.values())


def test_refusals_come_before_any_launch(hip_lib, gauss, binary):
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

    def refused(match, samplers=None, error=RuntimeError, **kw):
        before = live.get_counters()
        for smp in samplers or (live, gauss.stored[S]):
            with pytest.raises(error, match=match):
                smp.predict_loo(x, **{"y": y, "sigma": sg, **kw})
            assert smp.loo_info["launches"] == 0 and not any(smp.loo_info.values())
        assert np.array_equal(live.get_counters(), before), "a refused call launched something"
    for t in (4, 13, 1025, -1, 1):          # S = 13: the admissible tails are 5 .. 12
        refused(rf"tail_len {t} outside \[5, 12\]", tail_len=t)
    refused(r"tail_len 1025 outside \[5, 1024\]", tail_len=1025, peers=[gauss.stored[13]] * 100, peer_sigma=[sg] * 100)
    refused("NULL y", y=None)
    refused("outputs must name at least one of", error=ValueError, outputs=())
    for v in (0.0, -1.0, np.nan, np.inf):
        refused(r"sigma holds \S+ at draw 4 \(every sigma must be finite and > 0\)", sigma=bad(sg, 4, v))
        refused(r"peer_sigma\[0\] holds \S+ at draw 2", peers=[gauss.stored[5]], peer_sigma=[bad(np.ones(5), 2, v)])
    refused("link 0 needs sigma", sigma=None)
    refused("link 0 needs peer_sigma", peers=[gauss.stored[5]])
    for v in (-0.5, np.nan, np.inf):
        refused(r"row_scale holds \S+ at row 7 \(finite and >= 0\)", row_scale=bad(np.ones(rows), 7, v))
    refused("row_scale is 0 at row 7: with y every row_scale must be > 0", row_scale=bad(np.ones(rows), 7, 0.0))
    for v in (np.nan, np.inf, -np.inf):
        refused(r"y holds \S+ at row 9 \(every y must be finite\)", y=bad(y, 9, v))
    refused("under link 1 every y is 0 or 1", y=bad(y, 9, 2.0), link=1, sigma=None, samplers=(binary.stored[5],))
    refused("link must be 0", link=2)
    refused("negative scratch_bytes", scratch_bytes=-1)
    # the pool: 16 393 draws, and the peer rules of predict_quantiles
    with pytest.raises(RuntimeError, match="16393 pooled draws, at most 16384"):
        live.predict_loo(x[:3], y=y[:3], sigma=sg, peers=[gauss.stored[13]] * 1260, peer_sigma=[sg] * 1260)
    assert not any(live.loo_info.values())
    refused("peer 1 has 11 trees per draw, the sampler 25", peers=[gauss.stored[5], binary.stored[5]], peer_sigma=[np.ones(5)] * 2)
    refused("n_dense > 0 needs peer_dense_coef", peers=[gauss.stored[5]], peer_sigma=[np.ones(5)], dense=parts["dense"], dense_coef=parts["dense_coef"])
    refused("n_ell > 0 needs peer_ell_coef", peers=[gauss.stored[5]], peer_sigma=[np.ones(5)], peer_dense_coef=[peer["dense_coef"]], **parts)
    # the query form and a NULL output struct's neighbours: all output pointers NULL is a query, nothing is launched
    import ctypes as C
    from stan4bart_amd.abi import LooIn, LooOut, Sampler
    rows_in, keep, _, _ = Sampler._summary_in(S, x, None, None, None, None, None, None, 0, None, "auto", 0, 0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))          # noqa: E731
    before = live.get_counters()
    out = LooOut()
    assert hip_lib.s4b_predict_loo(live._h, C.byref(LooIn(rows=rows_in, y=dp(y), sigma=dp(sg))), C.byref(out)) == 0 and out.num_samples == S and not any(out.info)
    buf = np.zeros(rows)
    out = LooOut(ess=dp(buf))
    assert hip_lib.s4b_predict_loo(live._h, C.byref(LooIn(rows=rows_in, sigma=dp(sg))), C.byref(out)) == 1 and "NULL y" in hip_lib.s4b_last_error().decode()
    assert not any(out.info) and out.tail_len == 0 and np.array_equal(live.get_counters(), before)
    ok = live.predict_loo(x, y=y, sigma=sg, peers=[gauss.stored[5]], peer_sigma=[np.ones(5)], peer_dense_coef=[peer["dense_coef"]],
                          peer_ell_coef=[peer["ell_coef"]], **parts)
    assert ok["info"]["launches"] == 2 and live.get_counters()[2] == before[2] + 2 and ok["draws"] == 18
    del keep


def test_lpd_agrees_with_predict_ppd_within_the_two_bounds(gauss):
    """The same call through both entries: predict_ppd sums the draws in pooled order, predict_loo in sorted order — each within its own bound of the
    model's lpd, so within the sum of the two of each other; not bit for bit."""
    pool, rows = POOLS[65], 300
    got, (x, kw), (ref, bd, compared) = _case(gauss, pool, rows, "lpd against predict_ppd", M=1, E=1, offset=True, seed=65)
    x2, _, parts, row_side = _inputs(gauss, pool, rows, 1, 1, True, 65)
    pkw = {k: v for k, v in kw.items() if k != "tail_len"}
    ppd = gauss.stored[pool[0]].predict_ppd(x, (), moments=False, pit=False, **pkw)
    pref, pbd = pp.model(parts, y=kw["y"], row_scale=kw["row_scale"], **row_side)
    r = lc.bound_ratio(got["lpd"], ppd["lpd"], bd["lpd"] + pbd["lpd"])
    print(f"lpd of predict_loo against predict_ppd's: max |difference| / (sum of the two bounds) = {r:.3g}; equal bits in {np.mean(got['lpd'] == ppd['lpd']):.0%} of the rows")
    assert r <= lc.BOUND_FACTOR
    np.testing.assert_allclose(ref["lpd"], pref["lpd"], rtol=2.0 ** -50, atol=0.0, err_msg="the two models disagree on lpd")          # (long double sums in two orders, rounded once)


def test_whole_interface(hip_lib):
    """Stan4bartFit.predict_loo against fit.predict(type="ev") and extract("sigma") put through the numpy model: two chains, fixed effects, random
    intercepts, a continuous response, observation weights; the totals recomputed from the per-row results."""
    from stan4bart_amd import GroupTerm, generate_friedman_data
    from stan4bart_amd.abi import Sampler
    from stan4bart_amd.generics import combine_chains_f, stan4bart
    d = generate_friedman_data(120, ranef=True, causal=True, p=10)
    x = d["x"]
    xb, X = x[:, [j for j in range(10) if j != 3]], np.column_stack([x[:, 3], d["z"]])
    groups = [GroupTerm(d["g1"], None, "g.1"), GroupTerm(d["g2"], None, "g.2")]
    fit = stan4bart(d["y"], xb, X=X, groups=groups, chains=2, seed=99, iter=20, warmup=6, bart_args={"n.trees": 9, "keepTrees": True},
                    make_sampler=lambda a, st: Sampler(hip_lib, "s4b_", a, st))
    try:
        m = 50
        g = np.random.default_rng(3)
        new = [GroupTerm(np.asarray(d["g1"])[:m], None, "g.1"), GroupTerm(np.asarray(d["g2"])[:m], None, "g.2")]
        xb_new, X_new = xb[:m] + 0.01 * g.normal(size=(m, 9)), X[:m] + 0.05 * g.normal(size=(m, 2))
        y_new = np.asarray(d["y"], dtype=np.float64)[:m] + 0.5 * g.normal(size=m)
        w = g.uniform(0.5, 2.0, m)
        full = fit.predict(x_bart=xb_new, X=X_new, groups=new, type="ev", combine_chains=False, seed=7)          # [rows, iter, chain]
        assert full.shape == (m, 14, 2)
        flat, sigma = combine_chains_f(full), fit.extract("sigma")
        assert sigma.shape == (28,) and np.all(sigma > 0)
        ix, val, coef = fit._ell_random(new, True, np.random.default_rng(7))
        beta = fit.stan[fit._rows("beta.")]
        bart = np.concatenate([s.predict_bart(xb_new) for s in fit.samplers], axis=1)
        mref, mbound = sc.model(bart, None, X_new - fit.X_means, np.concatenate([beta[:, :, c].T for c in range(2)]), ix, val, np.concatenate(coef))
        assert sc.bound_ratio(flat, mref["v"], mbound["v"]) <= sc.BOUND_FACTOR, "fit.predict and the model over the ELL table describe different draws"
        got = fit.predict_loo(xb_new, X=X_new, groups=new, y=y_new, obs_weights=w, seed=7)
        assert got["draws"] == 28 and got["tail_len"] == lc.tail_len(28) == 6
        ref, bd, compared = lc.from_z(flat, 2.0 * np.broadcast_to(mbound["v"], flat.shape), sigma, y_new, None, 1.0 / np.sqrt(w), what="whole interface")
        for key in ("elpd_loo", "lpd", "ess"):
            r = lc.bound_ratio(got[key][compared], ref[key][compared], bd[key][compared])
            print(f"whole interface: {key}, max |device - model over fit.predict| / bound = {r:.3g}")
            assert r <= lc.BOUND_FACTOR, (key, r)
        fin = compared & np.isfinite(ref["pareto_k"])
        assert np.array_equal(np.isinf(got["pareto_k"])[compared], np.isinf(ref["pareto_k"])[compared]) and fin.sum() > 0.9 * m
        assert lc.bound_ratio(got["pareto_k"][fin], ref["pareto_k"][fin], bd["pareto_k"][fin]) <= lc.BOUND_FACTOR
        assert np.array_equal(got["p_loo"], got["lpd"] - got["elpd_loo"]) and got["elpd_loo_total"] == float(got["elpd_loo"].sum())
        assert got["p_loo_total"] == float(got["p_loo"].sum()) and got["se"] == pytest.approx(np.sqrt(m * np.var(got["elpd_loo"], ddof=1)), rel=1e-12)
        thr = min(1.0 - 1.0 / np.log10(28), 0.7)
        assert got["k_threshold"] == pytest.approx(thr) and got["n_high_k"] == int(np.sum(got["pareto_k"] > thr))
        again = fit.predict_loo(xb_new, X=X_new, groups=new, y=y_new, obs_weights=w, seed=7)
        assert all(np.array_equal(again[k], got[k]) for k in ("elpd_loo", "pareto_k", "lpd", "ess"))
        half = fit.predict_loo(xb_new, X=X_new, groups=new, y=y_new, obs_weights=w, r_eff=0.5, seed=7)
        assert half["tail_len"] == lc.tail_len_r_eff(28, 0.5) == 6
    finally:
        fit.close()
