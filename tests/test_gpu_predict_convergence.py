"""s4b_predict_convergence on the device (stan4bart_amd/csrc/dev_conv.inc: k_predict_values<staged / global> unchanged, k_chain_rows) against numpy on
the full pooled matrix (tests/conv_cases.py: the model, the bound, the rows left out).  Chain lengths 3 (no answer), 4 and 5 (the sequence stops at
pair 0), 6 and 7 (one trip), 8, 9, 13 beside 5 (cut), odd lengths split (the middle draw dropped); 1, 2, 4, 8 and 256 chains, 258 refused; the pair
the sequence stops at on either side of the first and the second block of 64 lags (31 / 32, 63 / 64) and at its limit; one, two and four waves per
row, one row per workgroup, 16 384 pooled draws; rows around a workgroup and a chunk; planted rows; both routes, live and stored samplers, two calls,
chunking — bit for bit; permuted peers — the same n_pairs, the values within the same bound (the sums over the chains run in chain order, so not the
same bits); the likelihood series (gaussian with row scales and a sigma vector per peer, binary, an underflow); the mean
against predict_summary's; the device bytes; the refusals before any launch; the whole Python interface.

Two small Friedman chains, as tests/test_gpu_predict_loo.py builds them: a short one with stored samplers of 3 .. 9 and 13 draws and a long one (5
trees) with 66, 68, 130, 132 and 2 048.  A handle is pooled repeatedly; every OCCURRENCE gets coefficient tables of its own, so the chains differ.
Series are planted through one-hot dense rows over per-draw dense_coef columns."""
import struct

import numpy as np
import pytest

import conv_cases as cc
import pd_cases as pc
import ppd_cases as pp
import readout_cases as rc
import summary_cases as sc

pytestmark = pytest.mark.gpu
WORST = {}
ZERO_PAIR = (0, -3, 2, 1, -2, 1, 2, -3, 2)          # N = 9, mean 0, q = 36, lag sums -18, -9, 18: rho = 1, -5/8, -3/8, 3/8 — P_1 = 0 EXACTLY, in double too
TAIL_TERM = (1, -3, -2, -4, 2, 0, 3, 1, 2)          # N = 9, q = 48: P_0 > 0.2, P_1 < -0.2 (zeroed), e_1 = 0.25 (the tail term); tau = 4 / 3


def _report(line):
    print(line)


def _note(ratios):
    for k, r in ratios.items():
        WORST[k] = max(WORST.get(k, 0.0), r)


class Chain(pc.Chain):
    """pd_cases.Chain on the product library, with predict_bart of every stored sampler at its rows (computed when first asked for)."""

    def __init__(self, lib, args, rows, steps):
        super().__init__(lib, "s4b_", args, steps=steps, rows=rows)
        self._bart = {}

    def bart(self, S):
        if S not in self._bart:
            self._bart[S] = self.stored[S].predict_bart(self.x)
        return self._bart[S]


@pytest.fixture(scope="module")
def short(hip_lib):
    c = Chain(hip_lib, rc._friedman(n=100, T=5, warmup=4, iter=17, ranef=False), rows=1100, steps=(3, 1, 1, 1, 1, 1, 1, 4))
    yield c
    c.close()
    print("predict_convergence, largest |device - model| / bound of this module: " + ", ".join(f"{k} {r:.3g}" for k, r in WORST.items()))


@pytest.fixture(scope="module")
def long(hip_lib):
    c = Chain(hip_lib, rc._friedman(n=100, T=5, warmup=4, iter=4 + 2048, ranef=False), rows=130, steps=(66, 2, 62, 2, 1916))
    yield c
    c.close()


@pytest.fixture(scope="module")
def binary(hip_lib):
    c = Chain(hip_lib, rc._binary(n=400, T=11, warmup=6, iter=19), rows=300, steps=(1, 1, 3, 8))
    yield c
    c.close()


class Plan:
    """The arguments of a pooled call over the first `rows` rows and the model's `parts`.  Ordinary rows: z = bart + w1 a + w2 b with per-occurrence
    series a (AR(1), phi 0.8, a small shift per occurrence) and b (white) and per-row weights.  `plant(i, series)`: row i gets z = bart + scale x
    series through a one-hot dense column.  `plant(i, series, exact=True)`: a first one-hot column whose coefficient at pooled draw k is -bart(i, k)
    takes the BART part out EXACTLY (bart + 1 x (-bart) = 0, then + 1 x series): the row's series is the planted one bit for bit."""

    def __init__(self, chain, lens, rows, seed=0, offset=None, amp=1.0):
        self.chain, self.lens, self.rows, self.S = chain, tuple(lens), rows, sum(lens)
        g = np.random.default_rng([6100, seed, len(lens), self.S])
        self.w = amp * g.uniform(0.0, 1.5, size=(rows, 2))
        a = np.concatenate([0.5 * cc.ar1(0.8, n, g) + 0.15 * g.standard_normal() for n in lens])
        self.cols = [a, 0.5 * g.standard_normal(self.S)]
        self.dense = [self.w[:, 0].copy(), self.w[:, 1].copy()]
        self.front = []          # (the cancelling columns go FIRST: the additions run in column order)
        self.offset = offset
        self.bart = np.concatenate([chain.bart(n)[:rows] for n in lens], axis=1)

    def plant(self, i, series, exact=False, scale=1.0):
        series = np.asarray(series, dtype=np.float64)
        assert series.shape == (self.S,)
        hot = np.zeros(self.rows)
        hot[i] = 1.0
        self.dense[0][i] = self.dense[1][i] = 0.0
        if exact:
            self.front.append((hot, -self.bart[i]))
        self.dense.append(hot)
        self.cols.append(scale * series)

    def build(self):
        dense = np.column_stack([h for h, _ in self.front] + self.dense)
        table = np.column_stack([c for _, c in self.front] + self.cols)          # [S x M]
        at = np.concatenate([[0], np.cumsum(self.lens)])
        tables = [np.ascontiguousarray(table[at[j]:at[j + 1]]) for j in range(len(self.lens))]
        kw = dict(offset=self.offset, dense=dense, dense_coef=tables[0], peers=[self.chain.stored[n] for n in self.lens[1:]], peer_dense_coef=tables[1:])
        parts = [dict(bart=self.chain.bart(n)[:self.rows], dense_coef=t) for n, t in zip(self.lens, tables)]
        return np.asfortranarray(self.chain.x[:self.rows]), kw, parts, dict(offset=self.offset, dense=dense)


def _shifted(lens, g, by=8.0):
    """White noise, the first pooled sampler's draws moved up by `by` sd: rhat >> 1, every rho near 1, the sequence runs to its limit."""
    s = g.standard_normal(sum(lens))
    s[:lens[0]] += by
    return s


_REF = {}


def _case(chain, name, rows, what, seed=0, plant=None, offset=None, lens=None, split=None, **call):
    """One pooled call against the model; the reference of a case is computed once and shared by the routes."""
    if lens is None:
        lens, split = cc.POOLS[name]
    plan = Plan(chain, lens, rows, seed, offset)
    if plant:
        plant(plan)
    x, kw, parts, row_side = plan.build()
    starts, N = cc.chains(lens, split)
    ck = (id(chain), name, rows, seed)
    if ck not in _REF:
        _REF[ck] = cc.model(parts, starts, N, what=what, **row_side)
    ref, bd, compared = _REF[ck]
    got = chain.stored[lens[0]].predict_convergence(x, split=split, **kw, **call)
    S = sum(lens)
    assert got["draws"] == S and got["info"]["draws"] == S and got["info"]["launches"] == 2 * got["info"]["chunks"]
    assert got["chains"] == len(starts) and got["chain_len"] == N
    _note(cc.assert_conv(got, ref, bd, compared, what, _report))
    return got, (x, dict(kw, split=split)), (ref, bd, compared)


def _same_bits(a, b, what, keys=cc.OUTPUTS + ("n_pairs",)):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k} differs"


@pytest.mark.parametrize("name", ["3", "4", "5", "6", "7", "8", "9", "13+5", "6s", "8s", "9s", "13s", "13+9s"])
def test_chain_lengths_after_the_cut_and_the_split(short, name):
    lens, split = cc.POOLS[name]
    rows = 130
    off = 2.0 * np.random.default_rng(sum(lens)).uniform(-1.0, 1.0, rows)
    off[17] = np.nan

    def plant(p):          # (called once per route: the same series both times)
        p.plant(5, _shifted(lens, np.random.default_rng(len(name) + sum(lens))), scale=30.0)
    res = {}
    for route in ("staged", "global"):
        res[route], _, (ref, bd, compared) = _case(short, name, rows, f"pool {name} {route}", plant=plant, offset=off, route=route)
        info = res[route]["info"]
        sp = 1 << (sum(lens) - 1).bit_length()
        assert info["route"] == (1 if route == "staged" else 2) and info["padded_draws"] == sp and info["rows_per_sort"] == 4096 // sp
    _same_bits(res["staged"], res["global"], f"pool {name}: the two routes")
    got, N = res["staged"], cc.chains(lens, split)[1]
    assert N == {"3": 3, "4": 4, "5": 5, "6": 6, "7": 7, "8": 8, "9": 9, "13+5": 5, "6s": 3, "8s": 4, "9s": 4, "13s": 6, "13+9s": 4}[name]
    assert np.isnan(got["ess"][17]) and got["n_pairs"][17] == -1, "the NaN offset does not leave its row without an answer"
    if N < 4:
        assert all(np.all(np.isnan(got[k])) for k in cc.OUTPUTS) and np.all(got["n_pairs"] == -1)
        return
    live = np.delete(np.arange(rows), 17)
    assert np.all(got["n_pairs"][live] <= cc.j_limit(N)) and got["n_pairs"][5] == cc.j_limit(N) and got["rhat"][5] > 2.0
    if N < 6:          # no trip of the loop: tau = 2 whatever the data
        assert np.all(got["n_pairs"][live] == 0) and np.array_equal(got["ess"][live], np.full(rows - 1, got["chains"] * N / 2.0))


@pytest.mark.parametrize("name,chains_", [("1x13", 1), ("1x13s", 2), ("4x13s", 8), ("128x9s", 256)])
def test_number_of_chains(short, name, chains_):
    lens, split = cc.POOLS[name]
    rows = 70

    def plant(p):
        g = np.random.default_rng(chains_)
        p.plant(9, _shifted(lens, g) if len(lens) > 1 else g.standard_normal(sum(lens)), scale=30.0)
    got, *_ = _case(short, name, rows, f"pool {name}", plant=plant, seed=chains_)
    assert got["chains"] == chains_
    if chains_ == 1:
        assert np.all(np.isnan(got["rhat"])) and np.all(np.isfinite(got["ess"])) and np.all(np.isfinite(got["mcse"]) | (got["ess"] < 0))
    else:
        assert np.all(got["rhat"] > 0.5)
    if chains_ == 256:
        assert got["info"]["padded_draws"] == 2048 and got["info"]["rows_per_sort"] == 2 and cc.lds_bytes(1152, 256) == 32768 + 128 + 8192 + 4096


def test_more_than_256_chains_are_refused_before_any_launch(short):
    x = np.asfortranarray(short.x[:5])
    smp = short.stored[9]
    before = short.live.get_counters()
    with pytest.raises(RuntimeError, match=r"258 chains, at most 256 \(129 pooled samplers, each split in two\)"):
        smp.predict_convergence(x, peers=[short.stored[9]] * 128)
    assert not any(smp.conv_info.values()) and np.array_equal(short.live.get_counters(), before)
    with pytest.raises(RuntimeError, match=r"257 chains, at most 256 \(257 pooled samplers\)"):
        smp.predict_convergence(x, split=False, peers=[short.stored[9]] * 256)
    assert not any(smp.conv_info.values())
    ok = smp.predict_convergence(x, split=False, peers=[short.stored[9]] * 255)
    assert ok["chains"] == 256 and ok["chain_len"] == 9 and ok["info"]["launches"] == 2


@pytest.mark.parametrize("name,limit", [("2x66", 31), ("2x68", 32), ("2x130", 63), ("2x132", 64), ("2x132s", 31)])
def test_the_pair_the_sequence_stops_at_around_the_blocks_of_lags(long, name, limit):
    """Pairs 0 .. 31 are the first block of 64 lags, 32 .. 63 the second.  The shifted row runs to the limit of its chain length — 31 (the last pair of
    the first block), 32 (the first of the second), 63, 64 —, the sticky rows (phi 0.99, 0.9) stop deep inside, the others within a few pairs."""
    lens, split = cc.POOLS[name]
    rows = 100
    N = cc.chains(lens, split)[1]
    assert cc.j_limit(N) == limit
    phis = {11: 0.5, 12: 0.9, 13: 0.99, 14: -0.7, 15: 0.99, 16: 0.9}

    def plant(p):
        g = np.random.default_rng(limit + len(name))
        p.plant(10, _shifted(lens, g), scale=30.0)
        for i, phi in phis.items():
            p.plant(i, np.concatenate([cc.ar1(phi, n, g) for n in lens]), scale=30.0 * np.sqrt(1.0 - phi * phi))
    got, _, (ref, bd, compared) = _case(long, name, rows, f"pool {name}", plant=plant, seed=limit)
    assert got["n_pairs"][10] == limit and got["rhat"][10] > 2.0
    assert compared[10] and all(compared[i] for i in phis), "a planted row is left out of the comparison"
    assert got["n_pairs"][13] >= 3 and 0.0 < got["ess"][13] < got["ess"][11], "the sticky row (phi 0.99) is not worth less than the one of phi 0.5"
    print(f"pool {name}: n_pairs of the planted rows (shifted, phi 0.5, 0.9, 0.99, -0.7, 0.99, 0.9): {got['n_pairs'][10:17].tolist()}; all rows: "
          f"{np.bincount(got['n_pairs'][got['n_pairs'] >= 0]).tolist()}")


@pytest.mark.parametrize("name,rows,per_row_waves", [("7x132", 40, 1), ("9x132", 40, 2), ("17x132", 20, 4), ("8x2048", 6, 4)])
def test_one_two_and_four_waves_per_row_up_to_the_lds_maximum(long, name, rows, per_row_waves):
    lens, split = cc.POOLS[name]
    def plant(p):
        g = np.random.default_rng(rows + per_row_waves)
        p.plant(1, np.concatenate([cc.ar1(0.99, n, g) for n in lens]), scale=30.0 * np.sqrt(1.0 - 0.99 ** 2))
        p.plant(2, _shifted(lens, g), scale=30.0)
    got, *_ = _case(long, name, rows, f"pool {name}", plant=plant, seed=rows)
    S = sum(lens)
    sp = 1 << (S - 1).bit_length()
    assert got["info"]["padded_draws"] == sp and got["info"]["rows_per_sort"] == max(1, 4096 // sp) == {1: 4, 2: 2, 4: 1}[per_row_waves]
    assert got["n_pairs"][2] == cc.j_limit(got["chain_len"])
    if name == "8x2048":
        assert S == 16384 and got["chains"] == 16 and got["chain_len"] == 1024 and got["n_pairs"][2] == 510 and cc.lds_bytes(S, 16) == 131072 + 128 + 256 + 2048


@pytest.mark.parametrize("rows", [127, 128, 129])
def test_rows_around_a_workgroup(short, rows):
    got, *_ = _case(short, "13s", rows, f"{rows} rows, 128 per workgroup", seed=rows)
    assert got["info"]["rows_per_sort"] == 128 and got["info"]["padded_draws"] == 32


def test_chunks_live_and_stored_samplers_permuted_peers_and_determinism(short):
    name, rows = "13+9s", 1037
    lens, S = cc.POOLS[name][0], 35
    whole, (x, kw), _ = _case(short, name, rows, f"{rows} rows in one chunk", seed=4, offset=np.random.default_rng(4).uniform(-1, 1, rows))
    assert whole["info"]["chunks"] == 1 and whole["info"]["rows_per_chunk"] == rows and whole["info"]["launches"] == 2
    smp = short.stored[lens[0]]
    for C, chunks in ((64, 17), (192, 6)):
        for route in ("staged", "global"):
            got = smp.predict_convergence(x, scratch_bytes=8 * S * C + 8 * S * 63, route=route, **kw)          # (rounded down to 64 rows)
            info = got["info"]
            assert (info["rows_per_chunk"], info["chunks"], info["launches"]) == (C, chunks, 2 * chunks), info
            _same_bits(got, whole, f"{rows} rows in chunks of {C}, {route}")
    per_row = ("offset", "dense")
    few = {k: (v[:130] if k in per_row else v) for k, v in kw.items()}
    tiny = smp.predict_convergence(x[:130], scratch_bytes=1, **few)
    assert tiny["info"]["rows_per_chunk"] == 64 and tiny["info"]["chunks"] == 3          # at least 64 rows per chunk
    _same_bits(tiny, {k: whole[k][:130] for k in cc.OUTPUTS + ("n_pairs",)}, "scratch_bytes 1")
    _same_bits(smp.predict_convergence(x, **kw), whole, "the same call twice")
    # the live sampler holds the kept trees of stored[13]: as the caller and as a peer it returns the stored sampler's bits
    _same_bits(short.live.predict_convergence(x, **kw), whole, "live and stored sampler as the caller")
    swapped = dict(kw, peers=[short.live if p is short.stored[13] else p for p in kw["peers"]])
    _same_bits(smp.predict_convergence(x, **swapped), whole, "a live sampler among the peers")
    # the peers in another order, each with its own table: the same chains, so the same answer — n_pairs equal, every value within the SAME bound of the
    # same model.  Not the same bits: the sums over the chains run in chain order, and an order-free sum would need a data-dependent order.
    perm = dict(kw, peers=kw["peers"][::-1], peer_dense_coef=kw["peer_dense_coef"][::-1])
    other = smp.predict_convergence(x, **perm)
    assert other["chains"] == whole["chains"] and other["chain_len"] == whole["chain_len"]
    ref, bd, compared = _REF[(id(short), name, rows, 4)]
    _note(cc.assert_conv(other, ref, bd, compared, "permuted peers against the same model", _report))
    assert np.array_equal(other["n_pairs"][compared], whole["n_pairs"][compared])
    # only the outputs asked for are formed, with the same bits
    part = smp.predict_convergence(x, outputs=("rhat", "n_pairs"), **kw)
    assert part["ess"] is None and part["mean"] is None and part["mcse"] is None
    _same_bits(part, whole, "two outputs of five", ("rhat", "n_pairs"))


def test_planted_rows_take_their_branch_per_row(short):
    """Four occurrences of the 9-draw sampler, unsplit: C = 4, N = 9, D = 36.  The exact rows carry the same series in every chain (B' = 0)."""
    lens, rows = (9,) * 4, 200
    rep = lambda s: np.tile(np.asarray(s, dtype=np.float64), 4)          # noqa: E731
    one_const = np.concatenate([np.full(9, 0.1), np.random.default_rng(98).standard_normal(27)])

    def plant(p):
        g = np.random.default_rng(99)
        p.plant(20, rep(ZERO_PAIR), exact=True)
        p.plant(21, rep(TAIL_TERM), exact=True)
        p.plant(22, np.full(36, 0.7), exact=True)
        p.plant(23, one_const, exact=True)
        p.plant(24, _shifted(lens, g), scale=30.0)
    off = np.zeros(rows)
    off[25] = np.nan
    got, _, (ref, bd, compared) = _case(short, "planted", rows, "planted rows", plant=plant, offset=off, lens=lens, split=False, seed=9)
    assert np.array_equal(ref["x"][20], rep(ZERO_PAIR)) and np.array_equal(ref["x"][22], np.full(36, 0.7)) and np.array_equal(ref["x"][23], one_const)
    # the pair sum that is exactly 0: the sequence stops at pair 1 and KEEPS it (0 >= 0); every operation is exact, so the device must return the values
    # themselves: tau = -1 + 2 (3/8 - 3/8) + 0 = -1
    assert ref["n_pairs"][20] == 1 and got["n_pairs"][20] == 1 and got["ess"][20] == -36.0 and got["mean"][20] == 0.0 and got["rhat"][20] == pytest.approx(np.sqrt(8.0 / 9.0), rel=1e-15)
    # the last pair zeroed, its even entry the tail term: tau = -1 + 2 P_0 + e_1 from the lag sums
    d = np.asarray(TAIL_TERM, dtype=np.float64)
    A = [float(d[:9 - t] @ d[t:]) for t in range(4)]
    rho = [a / A[0] - 1.0 / 8.0 for a in A]
    assert 1.0 + rho[1] > 0.2 and rho[2] + rho[3] < -0.2 and rho[2] > 0.2
    tau = -1.0 + 2.0 * (1.0 + rho[1]) + rho[2]
    assert tau == pytest.approx(4.0 / 3.0, rel=1e-15) and 36.0 / tau < 36.0 * np.log10(36.0)
    assert compared[21] and got["n_pairs"][21] == 1 and got["ess"][21] == pytest.approx(36.0 / tau, rel=1e-13)
    # every chain constant: no answer; one chain constant beside others: an answer
    assert not ref["answer"][22] and np.isnan(got["ess"][22]) and np.isnan(got["mean"][22]) and got["n_pairs"][22] == -1
    assert ref["answer"][23] and compared[23] and np.isfinite(got["ess"][23]) and got["n_pairs"][23] >= 0
    assert got["n_pairs"][24] == cc.j_limit(9) == 2 and got["rhat"][24] > 2.0
    assert not ref["answer"][25] and np.isnan(got["rhat"][25])
    ordinary = np.setdiff1d(np.arange(rows), [20, 21, 22, 23, 24, 25])
    assert np.all(np.isfinite(got["ess"][ordinary])) and np.all(got["n_pairs"][ordinary] >= 0), "the planted rows changed their neighbours"


def _lik_case(chain, lens, split, rows, seed, link=0, underflow=None):
    plan = Plan(chain, lens, rows, seed, amp=0.3 if link else 1.0)          # (link 1: |z| stays below 8, where ppd_cases.score's bound holds)
    x, kw, parts, row_side = plan.build()
    g = np.random.default_rng([8800, seed])
    z, _ = pp.pooled_z(parts, **row_side)
    starts, N = cc.chains(lens, split)
    if link:
        y = (np.arange(rows) % 2).astype(np.float64)
        ref, bd, compared = cc.model(parts, starts, N, quantity=1, y=y, link=1, what="likelihood, binary", **row_side)
        return x, dict(kw, y=y, link=1, split=split, quantity="lik"), (ref, bd, compared)
    sigmas = [g.uniform(0.5, 2.0, n) for n in lens]
    rs = g.uniform(0.5, 3.0, rows) * np.maximum(z.std(axis=1), 0.1)
    y = z.mean(axis=1) + (z.std(axis=1) + rs) * g.standard_normal(rows)
    if underflow is not None:          # a response AT one draw under a tiny row scale: the other draws' likelihoods underflow against it
        rs[underflow] = 1e-4 * z[underflow].std()
        y[underflow] = z[underflow, 3]
    for p, sg in zip(parts, sigmas):
        p["sigma"] = sg
    ref, bd, compared = cc.model(parts, starts, N, quantity=1, y=y, row_scale=rs, what="likelihood, gaussian", **row_side)
    return x, dict(kw, y=y, row_scale=rs, sigma=sigmas[0], peer_sigma=sigmas[1:], split=split, quantity="lik"), (ref, bd, compared)


def test_likelihood_series_gaussian_with_row_scales_and_a_sigma_vector_per_peer(short):
    lens, rows = (13, 9, 13), 200
    x, kw, (ref, bd, compared) = _lik_case(short, lens, True, rows, 31, underflow=40)
    assert np.sum(ref["x"][40] == 0.0) >= 30 and ref["x"][40, 3] == 1.0, "the likelihood of the planted row does not underflow in (nearly) every other draw"
    res = {}
    for route in ("staged", "global"):
        res[route] = short.stored[13].predict_convergence(x, route=route, **kw)
        _note(cc.assert_conv(res[route], ref, bd, compared, f"likelihood, gaussian, {route}", _report))
    _same_bits(res["staged"], res["global"], "quantity 1: the two routes")
    got = res["staged"]
    assert got["chains"] == 6 and got["chain_len"] == 4 and np.isfinite(got["ess"][40]) and np.all(got["mean"][ref["answer"]] > 0) and np.all(got["mean"][ref["answer"]] <= 1.0)
    # every peer's own sigma reached its draws: one sigma for all is another answer
    same = dict(kw, peer_sigma=[np.resize(kw["sigma"], len(s)) for s in kw["peer_sigma"]])
    other = short.stored[13].predict_convergence(x, **same)
    assert np.mean(other["mean"] != got["mean"]) > 0.9
    _same_bits(short.live.predict_convergence(x, **kw), got, "quantity 1: the live sampler")
    with pytest.raises(RuntimeError, match=r"row_scale is 0 at row 7"):
        short.stored[13].predict_convergence(x, **dict(kw, row_scale=np.where(np.arange(rows) == 7, 0.0, kw["row_scale"])))
    assert not any(short.stored[13].conv_info.values())


def test_likelihood_series_binary_and_the_value_under_the_probit_link(binary):
    assert binary.args.is_binary
    lens, rows = (13, 13), 150
    x, kw, (ref, bd, compared) = _lik_case(binary, lens, True, rows, 5, link=1)
    got = binary.stored[13].predict_convergence(x, **kw)
    _note(cc.assert_conv(got, ref, bd, compared, "likelihood, binary", _report))
    with pytest.raises(RuntimeError, match="under link 1 every y is 0 or 1"):
        binary.stored[13].predict_convergence(x, **dict(kw, y=np.where(np.arange(rows) == 17, 0.5, kw["y"])))
    assert not any(binary.stored[13].conv_info.values())
    # quantity 0 under link 1: the series is Phi(z), predict_summary's v
    plan = Plan(binary, lens, rows, 6, amp=0.3)
    x, kw, parts, row_side = plan.build()
    starts, N = cc.chains(lens, True)
    ref, bd, compared = cc.model(parts, starts, N, link=1, what="Phi(z)", **row_side)
    got = binary.stored[13].predict_convergence(x, link=1, **kw)
    _note(cc.assert_conv(got, ref, bd, compared, "quantity 0, link 1", _report))
    assert np.all(got["mean"] > 0.0) and np.all(got["mean"] < 1.0)


def test_mean_agrees_with_predict_summary_within_the_two_bounds(short):
    """Unsplit chains of equal length use every pooled draw: the mean is predict_summary's over the same draws, each occurrence summarised with its own
    table and the parts pooled (summary_cases.chan_pool)."""
    lens, rows = (13, 13, 13), 300
    plan = Plan(short, lens, rows, 12)
    x, kw, parts, row_side = plan.build()
    got = short.stored[13].predict_convergence(x, split=False, **kw)
    tables = [kw["dense_coef"]] + kw["peer_dense_coef"]
    pieces = []
    for t in tables:
        r = short.stored[13].predict_summary(x, dense=kw["dense"], dense_coef=t)
        pieces.append((r["draws"], r["mean"], r["m2"]))
    n, mean, m2 = sc.chan_pool(pieces)
    bound = 0.0
    for p in parts:
        _, b = sc.model(p["bart"], dense=row_side["dense"], dense_coef=p["dense_coef"])
        bound = np.maximum(bound, b["mean"])
    ref, bd, compared = cc.model(parts, *cc.chains(lens, False), what="mean against predict_summary", **row_side)
    r = cc.bound_ratio(got["mean"], mean, bd["mean"] + bound + 4.0 * cc.U * np.abs(mean))
    print(f"mean of predict_convergence against predict_summary's pooled mean: max |difference| / (sum of the two bounds) = {r:.3g}")
    assert n == 39 and r <= cc.BOUND_FACTOR
    sd, pos = np.sqrt(m2 / (n - 1)), got["ess"] > 0
    assert pos.mean() > 0.9
    np.testing.assert_allclose(got["mcse"][pos] * np.sqrt(got["ess"][pos]), sd[pos], rtol=1e-11)


def test_device_memory_of_a_call(short):
    name, rows = "13+9s", 700
    lens = cc.POOLS[name][0]
    got, (x, kw), _ = _case(short, name, rows, "device memory", seed=21, offset=np.zeros(rows), scratch_bytes=8 * 35 * 192)
    nodes = sum(struct.unpack_from("<Q", short.stored[S].export_bart_state(), 28)[0] for S in lens)
    want = cc.device_bytes_formula(short.P, rows, nodes, 35, short.T, True, 2, 0, 0, 192, 6, 0, 0, False, 4, True)
    assert got["info"]["rows_per_chunk"] == 192 and got["info"]["device_bytes"] == want, (got["info"], want)
    x2, kw2, _ = _lik_case(short, lens, True, rows, 22)
    lik = short.stored[13].predict_convergence(x2, outputs=("ess",), scratch_bytes=8 * 35 * 192, **kw2)
    want = cc.device_bytes_formula(short.P, rows, nodes, 35, short.T, False, 2, 0, 0, 192, 6, 1, 0, True, 1, False)
    assert lik["info"]["device_bytes"] == want, (lik["info"], want)


def test_refusals_come_before_any_launch(hip_lib, short, binary):
    rows, S = 50, 13
    x = np.asfortranarray(short.x[:rows])
    live = short.live
    y, sg = np.zeros(rows), np.ones(S)
    parts = sc.linear_parts(rows, S, 1, 2)
    peer = sc.linear_parts(rows, 5, 1, 2, seed=1)

    def bad(a, at, v):
        a = np.array(a, dtype=np.float64)
        a[at] = v
        return a

    def refused(match, samplers=None, error=RuntimeError, **kw):
        before = live.get_counters()
        for smp in samplers or (live, short.stored[S]):
            with pytest.raises(error, match=match):
                smp.predict_convergence(x, **kw)
            assert smp.conv_info["launches"] == 0 and not any(smp.conv_info.values())
        assert np.array_equal(live.get_counters(), before), "a refused call launched something"
    lik = dict(quantity="lik", y=y, sigma=sg)
    refused("NULL y", quantity="lik", sigma=sg)
    refused("quantity 0 takes no y", y=y)
    refused("quantity must be 0", quantity=2)
    refused("outputs must name at least one of", error=ValueError, outputs=())
    for v in (0.0, -1.0, np.nan, np.inf):
        refused(r"sigma holds \S+ at draw 4 \(every sigma must be finite and > 0\)", **dict(lik, sigma=bad(sg, 4, v)))
        refused(r"peer_sigma\[0\] holds \S+ at draw 2", peers=[short.stored[5]], peer_sigma=[bad(np.ones(5), 2, v)], **lik)
    refused("link 0 needs sigma", quantity="lik", y=y)
    refused("link 0 needs peer_sigma", peers=[short.stored[5]], **lik)
    for v in (-0.5, np.nan, np.inf):
        refused(r"row_scale holds \S+ at row 7 \(finite and >= 0\)", row_scale=bad(np.ones(rows), 7, v), **lik)
    for v in (np.nan, np.inf, -np.inf):
        refused(r"y holds \S+ at row 9 \(every y must be finite\)", **dict(lik, y=bad(y, 9, v)))
    refused("under link 1 every y is 0 or 1", quantity="lik", y=bad(y, 9, 2.0), link=1, samplers=(binary.stored[5],))
    refused("link must be 0", link=2)
    refused("negative scratch_bytes", scratch_bytes=-1)
    # the pool: 16 393 draws (the chain count is checked after the pool, so stay below 257 samplers: 128 x 130 does not exist here — 1260 x 13 does)
    with pytest.raises(RuntimeError, match="16393 pooled draws, at most 16384"):
        live.predict_convergence(x[:3], peers=[short.stored[13]] * 1260)
    assert not any(live.conv_info.values())
    refused("peer 1 has 11 trees per draw, the sampler 5", peers=[short.stored[5], binary.stored[5]])
    refused("n_dense > 0 needs peer_dense_coef", peers=[short.stored[5]], dense=parts["dense"], dense_coef=parts["dense_coef"])
    refused("n_ell > 0 needs peer_ell_coef", peers=[short.stored[5]], peer_dense_coef=[peer["dense_coef"]], **parts)
    # the query form: all output pointers NULL is a query, nothing is launched; a refusal leaves info, n_chains and chain_len zero
    import ctypes as C
    from stan4bart_amd.abi import ConvIn, ConvOut, Sampler
    rows_in, keep, _, _ = Sampler._summary_in(S, x, None, None, None, None, None, None, 0, None, "auto", 0, 0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))          # noqa: E731
    before = live.get_counters()
    out = ConvOut()
    assert hip_lib.s4b_predict_convergence(live._h, C.byref(ConvIn(rows=rows_in, split=1)), C.byref(out)) == 0 and out.num_samples == S and not any(out.info)
    buf = np.zeros(rows)
    out = ConvOut(ess=dp(buf))
    assert hip_lib.s4b_predict_convergence(live._h, C.byref(ConvIn(rows=rows_in, split=3)), C.byref(out)) == 1 and "split must be 0 or 1" in hip_lib.s4b_last_error().decode()
    assert not any(out.info) and out.n_chains == 0 and out.chain_len == 0 and np.array_equal(live.get_counters(), before)
    ok = live.predict_convergence(x, peers=[short.stored[5]], peer_dense_coef=[peer["dense_coef"]], peer_ell_coef=[peer["ell_coef"]], **parts)
    assert ok["info"]["launches"] == 2 and live.get_counters()[2] == before[2] + 2 and ok["draws"] == 18 and ok["chains"] == 4 and ok["chain_len"] == 2
    assert np.all(np.isnan(ok["ess"])) and np.all(ok["n_pairs"] == -1)          # chains of 2 draws: no answer
    one = short.stored[3].predict_convergence(x)          # 3 draws split: halves of ONE draw
    assert one["chain_len"] == 1 and np.all(np.isnan(one["rhat"]))
    del keep


def test_whole_interface(hip_lib):
    """Stan4bartFit.predict_convergence against fit.predict(type="ev") put through the numpy model: two chains, fixed effects, random intercepts, a
    continuous response; the summaries recomputed from the per-row results; the likelihood series with observation weights and r_eff."""
    from stan4bart_amd import GroupTerm, generate_friedman_data
    from stan4bart_amd.abi import Sampler
    from stan4bart_amd.generics import combine_chains_f, stan4bart
    d = generate_friedman_data(120, ranef=True, causal=True, p=10)
    x = d["x"]
    xb, X = x[:, [j for j in range(10) if j != 3]], np.column_stack([x[:, 3], d["z"]])
    groups = [GroupTerm(d["g1"], None, "g.1"), GroupTerm(d["g2"], None, "g.2")]
    fit = stan4bart(d["y"], xb, X=X, groups=groups, chains=2, seed=99, iter=30, warmup=6, bart_args={"n.trees": 9, "keepTrees": True},
                    make_sampler=lambda a, st: Sampler(hip_lib, "s4b_", a, st))
    try:
        m = 50
        g = np.random.default_rng(3)
        new = [GroupTerm(np.asarray(d["g1"])[:m], None, "g.1"), GroupTerm(np.asarray(d["g2"])[:m], None, "g.2")]
        xb_new, X_new = xb[:m] + 0.01 * g.normal(size=(m, 9)), X[:m] + 0.05 * g.normal(size=(m, 2))
        y_new = np.asarray(d["y"], dtype=np.float64)[:m] + 0.5 * g.normal(size=m)
        w = g.uniform(0.5, 2.0, m)
        full = fit.predict(x_bart=xb_new, X=X_new, groups=new, type="ev", combine_chains=False, seed=7)          # [rows, iter, chain]
        assert full.shape == (m, 24, 2)
        flat, sigma = combine_chains_f(full), fit.extract("sigma")
        ix, val, coef = fit._ell_random(new, True, np.random.default_rng(7))
        beta = fit.stan[fit._rows("beta.")]
        bart = np.concatenate([s.predict_bart(xb_new) for s in fit.samplers], axis=1)
        mref, mbound = sc.model(bart, None, X_new - fit.X_means, np.concatenate([beta[:, :, c].T for c in range(2)]), ix, val, np.concatenate(coef))
        assert sc.bound_ratio(flat, mref["v"], mbound["v"]) <= sc.BOUND_FACTOR, "fit.predict and the model over the ELL table describe different draws"
        got = fit.predict_convergence(xb_new, X=X_new, groups=new, seed=7)
        assert (got["chains"], got["chain_len"], got["draws"]) == (4, 12, 48)
        starts, N = cc.chains((24, 24), True)
        ref, bd, compared = cc.from_x(flat, 2.0 * np.broadcast_to(mbound["v"], flat.shape), starts, N, what="whole interface")
        for key in cc.OUTPUTS:
            r = cc.bound_ratio(got[key][compared], ref[key][compared], bd[key][compared])
            print(f"whole interface: {key}, max |device - model over fit.predict| / bound = {r:.3g}")
            assert r <= cc.BOUND_FACTOR, (key, r)
        assert np.array_equal(got["n_pairs"][compared], ref["n_pairs"][compared]) and compared.sum() >= 0.98 * m
        assert got["rhat_max"] == float(got["rhat"].max()) and got["ess_min"] == float(got["ess"].min())
        assert got["n_high_rhat"] == int(np.sum(got["rhat"] > 1.01)) and "r_eff" not in got
        assert fit.predict_convergence(xb_new, X=X_new, groups=new, rhat_threshold=1.2, seed=7)["n_high_rhat"] == int(np.sum(got["rhat"] > 1.2))
        again = fit.predict_convergence(xb_new, X=X_new, groups=new, seed=7)
        assert all(np.array_equal(again[k], got[k]) for k in cc.OUTPUTS + ("n_pairs",))
        whole = fit.predict_convergence(xb_new, X=X_new, groups=new, split=False, seed=7)
        assert (whole["chains"], whole["chain_len"], whole["draws"]) == (2, 24, 48)
        # the likelihood of held-out responses: r_eff per row, its median as predict_loo's scalar
        lik = fit.predict_convergence(xb_new, X=X_new, groups=new, quantity="lik", y=y_new, obs_weights=w, seed=7)
        sd = (1.0 / np.sqrt(w))[:, None] * sigma[None, :]
        sref, sbound = pp.score(flat, 2.0 * np.broadcast_to(mbound["v"], flat.shape), y_new, sd, 0)
        lx, lbx = cc.lik_series(sref["l"], sbound["l"])
        ref, bd, compared = cc.from_x(lx, lbx, starts, N, what="whole interface, likelihood")
        for key in cc.OUTPUTS:
            r = cc.bound_ratio(lik[key][compared], ref[key][compared], bd[key][compared])
            print(f"whole interface, likelihood: {key}, max |device - model| / bound = {r:.3g}")
            assert r <= cc.BOUND_FACTOR, (key, r)
        assert np.array_equal(lik["r_eff"], lik["ess"] / 48.0)
        r_eff = float(min(1.0, max(np.median(lik["r_eff"]), 1e-3)))
        assert fit.predict_loo(xb_new, X=X_new, groups=new, y=y_new, obs_weights=w, r_eff=r_eff, seed=7)["draws"] == 48
    finally:
        fit.close()
