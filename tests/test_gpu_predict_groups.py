"""s4b_predict_groups on the device (stan4bart_amd/csrc/dev_groups.inc: k_predict_values / k_contrast_values unchanged, k_level_reduce, k_level_fold,
k_level_rows, k_row_quantiles unchanged over the level matrix) against numpy in long double on the full matrix (tests/group_cases.py: the model, the
bound, the labels).  The smallest shapes at which the segmented reduction can go wrong: rows around one and two slabs of 64 and 1 100 rows with a level
of one row, a level that is one slab, levels meeting on a slab edge, a level over three slabs and one over a chunk edge (C = 64, 128, one chunk: the
same bits); L = rows against predict_quantiles and predict_contrast bit for bit; L = 1 against their averages; 1 .. 2 048 pooled draws, peers twice and
permuted; both routes, live and stored samplers, two calls; a series planted exactly with thresholds on a value and at +-inf; link 1 with one and two
arms and the arms swapped; empty levels and zero weights; the refusals before any launch; the device bytes; the Python interface.

Small Friedman chains, as tests/test_gpu_predict_convergence.py builds them: n = 100, 5 trees, stored samplers of 1, 7, 8, 9, 255, 257 and 2 048
draws; a binary chain (11 trees; 1, 2, 5 and 13 draws) for link 1."""
import struct

import numpy as np
import pytest

import contrast_cases as cc
import group_cases as gc
import pd_cases as pc
import quantile_cases as qc
import readout_cases as rc
import summary_cases as sc

pytestmark = pytest.mark.gpu
WORST = {}
PROBS = (0.025, 0.5, 0.975, 0.0, 1.0, 1.0 / 3.0)
FLOATS = ("draws", "mean", "m2", "quantiles", "p_above")
ALL = ("mean", "m2", "weight", "count", "draws")


def _report(line):
    print(line)


def _note(ratios):
    for k, r in ratios.items():
        WORST[k] = max(WORST.get(k, 0.0), r)


class Chain(pc.Chain):
    """pd_cases.Chain on the product library; predict_bart and the leaf sums of every (stored sampler, rows) computed when first asked for."""

    def __init__(self, lib, args, rows, steps):
        super().__init__(lib, "s4b_", args, steps=steps, rows=rows)
        self._bart, self._sums = {}, {}
        self.x = np.asfortranarray(self.x)

    def bart(self, S, key=None, x=None):
        if (S, key) not in self._bart:
            self._bart[S, key] = self.stored[S].predict_bart(self.x if x is None else x)
        return self._bart[S, key]

    def arm0(self, col):
        """Arm 0's rows: the rows with column `col` overwritten by training values of other rows."""
        x0 = self.x.copy()
        n = len(self.args.x_bart)
        x0[:, col] = self.args.x_bart[(np.arange(len(x0)) * 7 + col + 1) % n, col]
        return x0

    def sums(self, S, key, x, col):
        if (S, key, col) not in self._sums:
            self._sums[S, key, col] = cc.leaf_sums(self.trees[S], x, self.hit(S, [col]) if col is not None else np.zeros((S, self.T), dtype=bool))
        return self._sums[S, key, col]

    def used_column(self, S):
        return int(np.argmax([self.hit(S, [j]).sum() for j in range(self.P)]))


@pytest.fixture(scope="module")
def gauss(hip_lib):
    c = Chain(hip_lib, rc._friedman(n=100, T=5, warmup=4, iter=4 + 2048, ranef=False), rows=1100, steps=(1, 6, 1, 1, 246, 2, 1791))
    yield c
    c.close()
    print("predict_groups, largest |device - model| / bound of this module: " + ", ".join(f"{k} {r:.3g}" for k, r in WORST.items()))


@pytest.fixture(scope="module")
def binary(hip_lib):
    c = Chain(hip_lib, rc._binary(n=400, T=11, warmup=6, iter=19), rows=300, steps=(1, 1, 3, 8))
    yield c
    c.close()


_REF = {}


def _values(chain, lens, rows, arms=1, link=0, M=0, offset=False, col=None, dense0=False, swap=False, seed=0):
    """The keyword arguments of a pooled call over the first `rows` rows and the reference matrix x with its bound.  Every OCCURRENCE of a pooled
    sampler gets a coefficient table of its own.  Two arms: column `col` of the BART rows differs (None: no BART column), `dense0`: arm 0 has a dense
    part of its own; `swap` exchanges the arms."""
    key = (id(chain), tuple(lens), rows, arms, link, M, offset, col, dense0, swap, seed)
    if key in _REF:
        return _REF[key]
    x1 = np.asfortranarray(chain.x[:rows])
    tables = [sc.linear_parts(rows, S, M, 0, seed=seed + 100 * j) for j, S in enumerate(lens)]
    shared = tables[0]
    off = float(chain.range[1] - chain.range[0]) * np.random.default_rng(seed).uniform(-1.0, 1.0, rows) if offset else None
    kw = dict(x_test=x1, offset=off, link=link, peers=[chain.stored[S] for S in lens[1:]], n_arms=arms, **shared)
    if M:
        kw["peer_dense_coef"] = [t["dense_coef"] for t in tables[1:]]
    if arms == 1:
        parts = [dict(bart=chain.bart(S)[:rows], dense_coef=t.get("dense_coef")) for S, t in zip(lens, tables)]
        _, _, v, bv = qc.model(parts, (), link=link, offset=off, dense=shared.get("dense"))
        # (predict_bart's value enters quantile_cases' model as an exact term; the device's k_predict_values forms the same sum bit for bit)
        _REF[key] = kw, v, bv
        return _REF[key]
    x0full = chain.arm0(col) if col is not None else chain.x
    x0 = np.asfortranarray(x0full[:rows])
    other = sc.linear_parts(rows, 1, M, 0, seed=seed + 50)
    arm1, a0 = dict(offset=off, dense=shared.get("dense")), dict(dense=other["dense"] if dense0 else None)
    parts = []
    for S, t in zip(lens, tables):
        cols = [col] if col is not None else []
        if cols:
            (F1, G1), (F0, G0) = chain.sums(S, None, chain.x, col), chain.sums(S, ("arm0", col), x0full, col)
            n_aff = chain.hit(S, cols).sum(axis=1)
        else:          # no BART column differs: no tree is affected
            (F1, G1), n_aff = chain.sums(S, None, chain.x, None), np.zeros(S, dtype=np.int64)
            F0, G0 = F1, G1
        parts.append(dict(bart1=chain.bart(S)[:rows], bart0=chain.bart(S, ("arm0", col), x0full)[:rows] if cols else chain.bart(S)[:rows], F1=F1[:rows], F0=F0[:rows],
                          G1=G1[:rows], G0=G0[:rows], n_affected=n_aff, dense_coef=t.get("dense_coef")))
    kw.update(x_test0=x0 if col is not None else None, dense0=a0["dense"])
    if swap:          # arm 1 <-> arm 0: both sides of every part that differs
        kw["x_test"], kw["x_test0"] = (x0, x1) if col is not None else (x1, None)
        if dense0:
            kw["dense"], kw["dense0"] = kw["dense0"], kw["dense"]
            arm1, a0 = dict(offset=off, dense=kw["dense"]), dict(dense=kw["dense0"])
        parts = [dict(p, bart1=p["bart0"], bart0=p["bart1"], F1=p["F0"], F0=p["F1"], G1=p["G0"], G0=p["G1"]) for p in parts]
    ref, bd = cc.model(parts, arm1, a0, chain.T, chain.range, chain.binary, link=link)
    _REF[key] = kw, ref["d"], bd["d"]
    return _REF[key]


def _case(chain, lens, rows, level, L, what, weights=None, statistic="mean", probs=PROBS, threshold="midway", outputs=ALL, values=None, **call):
    """One pooled call against the model.  `level` non-decreasing; threshold "midway": between two adjacent reference values."""
    kw, x, bx = _values(chain, lens, rows, **(values or {}))
    stat = gc_stat(statistic)
    if threshold == "midway":
        ref0, _ = gc.model(x, bx, level, L, weights, stat)
        threshold = gc.midway(ref0["draws"])
    ref, bd = gc.model(x, bx, level, L, weights, stat, probs, threshold)
    got = chain.stored[lens[0]].predict_groups(level=level, n_levels=L, weights=weights, statistic=statistic, probs=probs, threshold=threshold, outputs=outputs,
                                               presorted=True, **kw, **call)
    S, info = sum(lens), got["info"]
    assert got["draws_pooled"] == S and info["draws"] == S and info["edge_levels"] == gc.edge_levels(level, L), info
    _note(gc.assert_groups(got, ref, bd, what, _report))
    return got, (ref, bd), dict(kw, level=level, n_levels=L, weights=weights, statistic=statistic, probs=probs, threshold=threshold, outputs=outputs, presorted=True)


def gc_stat(statistic):
    return {"sum": 0, "mean": 1}[statistic]


def _same_bits(a, b, what, keys=FLOATS + ("weight", "count")):
    for k in keys:
        assert (a.get(k) is None) == (b.get(k) is None), (what, k)
        if a.get(k) is not None:
            assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k} differs"


# ---- slab edges ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [63, 64, 65, 129, 1100])
def test_slab_edges_and_chunking(gauss, rows):
    level, L = gc.slab_labels(rows)
    S = 9
    w = np.random.default_rng(rows).uniform(0.0, 2.0, rows)
    res = {}
    for name, scratch in (("C 64", 64 * 8 * S), ("C 128", 128 * 8 * S), ("one chunk", 0)):
        res[name], _, _ = _case(gauss, (S,), rows, level, L, f"{rows} rows, {name}", weights=w, values=dict(M=2, offset=True), scratch_bytes=scratch)
        info = res[name]["info"]
        C = min(rows, {"C 64": 64, "C 128": 128}.get(name, rows))
        assert info["rows_per_chunk"] == C and info["chunks"] == -(-rows // C), info
        assert info["nan_levels"] == (3 if rows > 64 else 2), info
    _same_bits(res["C 64"], res["C 128"], f"{rows} rows: C 64 and C 128")
    _same_bits(res["C 64"], res["one chunk"], f"{rows} rows: C 64 and one chunk")
    if rows == 1100:
        assert res["C 64"]["info"]["chunks"] == 18 and res["C 64"]["info"]["edge_levels"] >= 2
        assert res["C 64"]["info"]["launches"] > res["one chunk"]["info"]["launches"]
        sums, _, _ = _case(gauss, (S,), rows, level, L, "1100 rows, sums, no weights", statistic="sum", values=dict(M=2, offset=True), scratch_bytes=64 * 8 * S)
        assert np.array_equal(sums["weight"], sums["count"].astype(np.float64))


# ---- L = rows and L = 1 ----------------------------------------------------------------------------------------------------------------------------------
def test_every_row_its_own_level_is_the_row_bit_for_bit(gauss):
    rows, lens = 300, (9, 7)
    level = np.arange(rows)
    kw, _, _ = _values(gauss, lens, rows, M=2, offset=True)
    got, _, _ = _case(gauss, lens, rows, level, rows, "L = rows, one arm", statistic="sum", values=dict(M=2, offset=True))
    q = gauss.stored[9].predict_quantiles(probs=PROBS, **{k: v for k, v in kw.items() if k != "n_arms"})
    assert np.array_equal(got["quantiles"], q["quantiles"]), "a level of one row with weight 1 is not the row's value"
    col = gauss.used_column(9)
    kw2, _, _ = _values(gauss, lens, rows, arms=2, M=2, col=col, dense0=True)
    two, _, _ = _case(gauss, lens, rows, level, rows, "L = rows, two arms", statistic="sum", values=dict(arms=2, M=2, col=col, dense0=True))
    c = gauss.stored[9].predict_contrast(probs=PROBS, **{k: v for k, v in kw2.items() if k != "n_arms"})
    for k in ("mean", "m2", "quantiles"):
        assert np.array_equal(two[k], c[k]), f"L = rows, two arms: {k} is not predict_contrast's"
    mean, _, _ = _case(gauss, lens, rows, level, rows, "L = rows, mean", statistic="mean", values=dict(M=2, offset=True))
    _same_bits(got, mean, "a level of one row: the sum and the mean (the division by 1)", keys=FLOATS)


def test_one_level_against_the_averages(gauss):
    rows, lens = 1100, (9,)
    level, w = np.zeros(rows, dtype=np.int64), np.full(rows, 1.0 / rows)
    got, (ref, bd), _ = _case(gauss, lens, rows, level, 1, "L = 1, one arm", weights=w, statistic="sum", values=dict(M=2, offset=True))
    kw, _, _ = _values(gauss, lens, rows, M=2, offset=True)
    s = gauss.stored[9].predict_summary(weights=w[None, :], **{k: v for k, v in kw.items() if k not in ("n_arms", "peers", "peer_dense_coef")})
    # predict_summary adds the same terms in another order (wave butterfly, waves, tiles, workgroups): summary_cases' bound of its average
    _, x, bx = _values(gauss, lens, rows, M=2, offset=True)
    b2 = w @ bx + rows * gc.U * (w @ np.abs(x))
    r = gc.bound_ratio(got["draws"][0], s["average"][:, 0], bd["draws"][0] + b2)
    print(f"L = 1 against predict_summary's average: {r:.3g} x the sum of both bounds")
    assert r <= gc.BOUND_FACTOR
    col = gauss.used_column(9)
    two, (ref2, bd2), _ = _case(gauss, lens, rows, level, 1, "L = 1, two arms", weights=w, statistic="sum", values=dict(arms=2, col=col))
    kw2, _, _ = _values(gauss, lens, rows, arms=2, col=col)
    c = gauss.stored[9].predict_contrast(weights=w[None, :], **{k: v for k, v in kw2.items() if k != "n_arms"})
    # the same slabs and the same order inside them: the two calls differ only in the association of the fold over the slabs; each lies within the
    # model's bound of the model, so they lie within twice the bound of one another
    r = gc.bound_ratio(two["draws"][0], c["average"][:, 0], 2.0 * bd2["draws"][0])
    print(f"L = 1 against predict_contrast's average: {r:.3g} x twice the bound")
    assert r <= gc.BOUND_FACTOR and two["info"]["edge_levels"] == 1


# ---- draw counts -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 7, 8, 9, 255, 257, 2048])
def test_draw_counts(gauss, S):
    rows = 130
    level, L = gc.slab_labels(rows)
    got, _, _ = _case(gauss, (S,), rows, level, L, f"{S} draws", weights=np.random.default_rng(S).uniform(0.5, 1.5, rows), values=dict(M=1))
    if S == 1:
        ok = ~np.isnan(got["mean"])
        assert np.all(got["m2"][ok] == 0.0) and np.array_equal(got["mean"][ok], got["draws"][ok, 0])
    if S in (1, 9, 257):          # (the level kernels do not know the arms; the model's leaf sums of both arms are the slow part)
        two, _, _ = _case(gauss, (S,), rows, level, L, f"{S} draws, two arms", values=dict(arms=2, col=gauss.used_column(S)))
        if S == 1:
            assert np.all(two["m2"][~np.isnan(two["mean"])] == 0.0)


def test_peers_twice_and_permuted(gauss):
    rows = 130
    level, L = gc.slab_labels(rows)
    _case(gauss, (7, 7, 9), rows, level, L, "peers twice", values=dict(M=1))
    a, _, _ = _case(gauss, (7, 9), rows, level, L, "peers 7, 9")
    b, _, _ = _case(gauss, (9, 7), rows, level, L, "peers 9, 7", threshold=None)
    perm = np.r_[np.arange(7, 16), np.arange(7)]          # (9, 7)'s pooled draw k is (7, 9)'s draw perm[k]
    assert np.array_equal(a["draws"][:, perm], b["draws"], equal_nan=True), "permuted peers do not give the same values up to the permutation of the draws"
    assert np.array_equal(a["quantiles"], b["quantiles"], equal_nan=True), "permuted peers: the quantiles differ"


# ---- routes and samplers ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arms", [1, 2])
def test_routes_live_and_stored_two_calls(binary, arms):
    rows, S = 300, 13
    level, L = gc.slab_labels(rows)
    values = dict(arms=arms, M=1, **(dict(col=binary.used_column(S)) if arms == 2 else {}))
    res = {}
    for route in ("staged", "global"):
        res[route], _, call = _case(binary, (S,), rows, level, L, f"{arms} arm(s), {route}", values=values, route=route)
        assert res[route]["info"]["route"] == (1 if route == "staged" else 2)
    _same_bits(res["staged"], res["global"], "the two routes")
    again = binary.stored[S].predict_groups(**call, route="global")
    _same_bits(res["global"], again, "two calls")
    live = binary.live.predict_groups(**call)
    _same_bits(res["staged"], live, "live and stored samplers")


# ---- an exactly planted series ---------------------------------------------------------------------------------------------------------------------------
def test_planted_series_ties_and_infinite_thresholds(gauss):
    rows, S, i = 130, 9, 70
    series = np.array([0.5, -1.25, 3.0, 0.5, 2.0, -0.75, 3.0, 1.5, 0.0])
    bart = gauss.bart(S)[:rows]
    hot = np.zeros(rows)
    hot[i] = 1.0
    # the first one-hot column takes the BART part out exactly (bart + 1 x (-bart) = 0), the second adds the series: row i is the series bit for bit
    dense, coef = np.column_stack([hot, hot]), np.column_stack([-bart[i], series])
    level = np.r_[np.zeros(i, dtype=np.int64), [1], np.full(rows - i - 1, 2)]
    smp = gauss.stored[S]
    kw = dict(x_test=np.asfortranarray(gauss.x[:rows]), level=level, n_levels=3, dense=dense, dense_coef=coef, presorted=True, outputs=ALL, probs=(0.0, 0.5, 1.0))
    got = smp.predict_groups(threshold=1.5, **kw)
    assert np.array_equal(got["draws"][1], series), "the planted series did not arrive bit for bit"
    assert got["p_above"][1] == 3.0 / 9.0, "a draw equal to the threshold was counted (the comparison is strict)"
    assert np.array_equal(got["quantiles"][:, 1], [-1.25, 0.5, 3.0]) and got["mean"][1] == series.sum() / 9.0
    assert smp.predict_groups(threshold=3.0, **kw)["p_above"][1] == 0.0 and smp.predict_groups(threshold=-1.25, **kw)["p_above"][1] == 8.0 / 9.0
    assert np.array_equal(smp.predict_groups(threshold=np.inf, **kw)["p_above"], [0.0, 0.0, 0.0])
    assert np.array_equal(smp.predict_groups(threshold=-np.inf, **kw)["p_above"], [1.0, 1.0, 1.0])
    assert smp.predict_groups(**kw)["p_above"] is None
    sums = smp.predict_groups(threshold=1.5, statistic="sum", **kw)
    assert np.array_equal(sums["draws"][1], series) and sums["p_above"][1] == 3.0 / 9.0


# ---- link 1 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_link_1_one_arm_two_arms_and_swapped_arms(binary):
    """Swapping the arms negates every d bit for bit, so every sum, A, the mean and m2 (the same), and those quantiles whose formula is symmetric: the
    probs 0 and 1 change places, and the median of an ODD number of draws is one order statistic (g = 0).  An interpolated quantile x(lo) + g (x(hi) -
    x(lo)) is not the negative of the one formed from the other end, so it is not compared.  23 pooled draws."""
    rows, lens = 300, (5, 13, 5)
    level, L = gc.slab_labels(rows)
    w = np.random.default_rng(5).uniform(0.0, 1.0, rows)
    _case(binary, lens, rows, level, L, "link 1, one arm", weights=w, values=dict(link=1, M=2, offset=True))
    col = binary.used_column(13)
    for name, values in (("a BART column", dict(arms=2, link=1, M=2, col=col)), ("a dense column only", dict(arms=2, link=1, M=2, dense0=True))):
        a, (ref, _), call = _case(binary, lens, rows, level, L, f"link 1, two arms, {name}", weights=w, values=values)
        t = call["threshold"]
        b, _, _ = _case(binary, lens, rows, level, L, f"link 1, two arms, {name}, swapped", weights=w, values=dict(values, swap=True), threshold=-t)
        ok = ~np.isnan(a["mean"])
        assert ok.sum() >= 5 and np.any(a["draws"][ok] != 0.0)
        assert np.array_equal(b["draws"][ok], -a["draws"][ok]) and np.array_equal(b["mean"][ok], -a["mean"][ok]), f"{name}: swapped arms do not negate bit for bit"
        assert np.array_equal(b["m2"][ok], a["m2"][ok])
        q0, q1, med = PROBS.index(0.0), PROBS.index(1.0), PROBS.index(0.5)
        assert np.array_equal(b["quantiles"][q0, ok], -a["quantiles"][q1, ok]) and np.array_equal(b["quantiles"][q1, ok], -a["quantiles"][q0, ok])
        assert np.array_equal(b["quantiles"][med, ok], -a["quantiles"][med, ok])
        assert not np.any(ref["draws"][ok] == t), "a value ties with the threshold: the mirror below does not hold"
        assert np.array_equal(np.round(b["p_above"][ok] * 23), 23 - np.round(a["p_above"][ok] * 23)), f"{name}: p_above(-threshold) does not mirror"


# ---- empty levels and zero weights -----------------------------------------------------------------------------------------------------------------------
def test_empty_levels_and_zero_weights(gauss):
    rows, S = 130, 9
    level = np.r_[np.full(40, 1), np.full(30, 3), np.full(60, 4)].astype(np.int64)          # levels 0, 2 and 5 are empty; level 3 straddles row 64
    w = np.random.default_rng(3).uniform(0.5, 1.5, rows)
    w[40:70] = 0.0
    mean, _, _ = _case(gauss, (S,), rows, level, 6, "empty levels, zero weights, mean", weights=w, values=dict(M=1))
    assert mean["info"]["nan_levels"] == 4 and np.array_equal(np.isnan(mean["mean"]), [True, False, True, True, False, True])
    assert all(np.all(np.isnan(mean[k][..., [0, 2, 3, 5]])) for k in ("mean", "m2", "quantiles", "p_above")) and np.all(np.isnan(mean["draws"][[0, 2, 3, 5]]))
    assert np.array_equal(mean["weight"][[0, 2, 3, 5]], [0.0, 0.0, 0.0, 0.0]) and np.array_equal(mean["count"], [0, 40, 0, 30, 60, 0])
    sums, _, _ = _case(gauss, (S,), rows, level, 6, "empty levels, zero weights, sum", weights=w, statistic="sum", threshold=0.5, values=dict(M=1))
    assert sums["info"]["nan_levels"] == 3
    assert np.all(sums["draws"][3] == 0.0) and sums["mean"][3] == 0.0 and sums["m2"][3] == 0.0 and np.all(sums["quantiles"][:, 3] == 0.0) and sums["p_above"][3] == 0.0


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(gauss):
    rows, S = 300, 9
    x = np.asfortranarray(gauss.x[:rows])
    level, L = gc.slab_labels(rows)
    live, smp = gauss.live, gauss.stored[S]
    own = live.groups_draws()

    def refused(match, **kw):
        before = live.get_counters()
        for s in (live, smp):
            args = dict(x_test=x, level=level, n_levels=L, presorted=True, probs=(0.5,))
            args.update(kw)
            with pytest.raises(RuntimeError, match=match):
                s.predict_groups(**args)
            assert not any(s.groups_info.values()), s.groups_info
        assert np.array_equal(live.get_counters(), before), "a refused call launched something"

    def changed(i, v):
        out = level.copy()
        out[i] = v
        return out
    refused("predict_groups: the levels decrease at row 5", level=changed(4, 3))
    refused(f"predict_groups: level {L} of row {rows - 1} outside", level=changed(rows - 1, L))
    refused("predict_groups: level -1 of row 0 outside", level=changed(0, -1))
    for bad, name in ((-1.0, "-1"), (np.nan, "nan"), (np.inf, "inf")):
        w = np.ones(rows)
        w[17] = bad
        refused(f"predict_groups: weight {name}.* of row 17 is negative or not finite", weights=w)
    refused("predict_groups: n_arms must be 1 .* or 2 .*, not 0", n_arms=0)
    refused("predict_groups: n_arms must be 1 .* or 2 .*, not 3", n_arms=3)
    refused("predict_groups: n_arms = 1 takes no arm-0 pointer", x_test0=x)
    refused("predict_groups: n_arms = 1 takes no arm-0 pointer", offset=np.zeros(rows), offset0=np.zeros(rows))
    refused("predict_groups: statistic must be 0 .* or 1", statistic=2)
    for s, draws in ((live, own), (smp, S)):
        before = live.get_counters()
        with pytest.raises(RuntimeError, match=f"predict_groups: the level matrix of {L} levels x {draws} pooled draws exceeds {8 * (L - 1) * draws} bytes"):
            s.predict_groups(x_test=x, level=level, n_levels=L, presorted=True, level_bytes=8 * (L - 1) * draws)
        assert not any(s.groups_info.values()) and np.array_equal(live.get_counters(), before)
    ok = smp.predict_groups(x_test=x, level=level, n_levels=L, presorted=True, level_bytes=8 * L * S, probs=(0.5,))
    assert gc.edge_levels(level, L) > 0 and ok["info"]["launches"] == 5, ok["info"]          # values, reduce, fold; level rows, sort
    before = live.get_counters()
    live.predict_groups(x_test=x, level=level, n_levels=L, presorted=True)
    assert live.get_counters()[2] == before[2] + 4


# ---- device bytes ----------------------------------------------------------------------------------------------------------------------------------------
def test_device_bytes(gauss):
    rows, S, T = 1100, 9, gauss.T
    level, L = gc.slab_labels(rows)
    nodes = struct.unpack_from("<Q", gauss.stored[S].export_bart_state(), 28)[0]
    w = np.ones(rows)
    got, _, _ = _case(gauss, (S,), rows, level, L, "device bytes, one arm", weights=w, values=dict(M=2, offset=True), scratch_bytes=128 * 8 * S)
    C, Q = got["info"]["rows_per_chunk"], len(PROBS)
    assert C == 128
    value = qc.device_bytes_formula(gauss.P, rows, nodes, S, T, True, 2, 0, 0, C, 0) - 2 * 16          # (no quantiles per row, no probs there)
    want = gc.device_bytes_formula(value, rows, S, L, C, weights=True, p_above=True, Q=Q, edge=gc.edge_levels(level, L))
    print(f"device memory of the call: {got['info']['device_bytes']} bytes, the sum of DESIGN.md 5.12: {want}; the draws matrix would take {8 * rows * S}")
    assert got["info"]["device_bytes"] == want
    col = gauss.used_column(S)
    two, _, _ = _case(gauss, (S,), rows, level, L, "device bytes, two arms", values=dict(arms=2, col=col), scratch_bytes=128 * 8 * S)
    value = cc.device_bytes_formula(gauss.P, rows, nodes, S, T, 128, D=1, per_row=False)
    want = gc.device_bytes_formula(value, rows, S, L, 128, p_above=True, Q=Q, edge=gc.edge_levels(level, L))
    assert two["info"]["device_bytes"] == want, (two["info"], want)


# ---- the Python interface --------------------------------------------------------------------------------------------------------------------------------
def test_whole_interface(hip_lib):
    """Stan4bartFit.predict_groups against a numpy group-by over fit.predict of the same seed: unsorted string labels, by="g.1", treatment=, return_draws
    with and without combine_chains, a split of the levels into several calls."""
    from stan4bart_amd import GroupTerm, generate_friedman_data
    from stan4bart_amd.abi import Sampler
    from stan4bart_amd.generics import combine_chains_f, stan4bart
    d = generate_friedman_data(120, ranef=True, causal=True, p=10)
    x, z = d["x"], np.asarray(d["z"], dtype=np.float64)
    xb, X = np.column_stack([x[:, [j for j in range(10) if j != 3]], z]), np.column_stack([x[:, 3], z])
    groups = [GroupTerm(d["g1"], None, "g.1"), GroupTerm(d["g2"], None, "g.2")]
    fit = stan4bart(d["y"], xb, X=X, groups=groups, chains=2, seed=99, iter=14, warmup=6, bart_args={"n.trees": 9, "keepTrees": True},
                    make_sampler=lambda a, st: Sampler(hip_lib, "s4b_", a, st))
    try:
        m = 90
        g = np.random.default_rng(11)
        xb1, X1, off = rc.new_rows(xb, m, seed=4), X[:m] + g.normal(size=(m, 2)), g.normal(size=m)
        new = [GroupTerm(np.asarray(d["g1"])[:m], None, "g.1"), GroupTerm(np.asarray(d["g2"])[:m], None, "g.2")]
        names = np.array(["north", "south", "east", "west", "centre", "isle", "coast"])
        by = names[g.integers(0, len(names), m)]          # unsorted string labels
        w = g.uniform(0.0, 2.0, m)
        full = fit.predict(x_bart=xb1, X=X1, groups=new, offset=off, combine_chains=False, seed=7)          # [rows, iter, chain]
        flat = combine_chains_f(full)
        probs = (0.025, 0.5, 0.975)
        got = fit.predict_groups(by, xb1, X=X1, groups=new, offset=off, row_weights=w, probs=probs, return_draws=True, seed=7)
        lab = np.unique(by)
        assert np.array_equal(got["levels"], lab) and got["draws"] == 16 and got["average"].shape == (len(lab), 16)
        want = np.vstack([(w[by == l, None] * flat[by == l]).sum(axis=0) / w[by == l].sum() for l in lab])
        np.testing.assert_allclose(got["average"], want, rtol=1e-11, atol=1e-12)
        np.testing.assert_allclose(got["mean"], want.mean(axis=1), rtol=1e-11, atol=1e-12)
        np.testing.assert_allclose(got["sd"], want.std(axis=1, ddof=1), rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(got["quantiles"], np.quantile(want, probs, axis=1), rtol=1e-11, atol=1e-12)
        assert np.array_equal(got["count"], [np.sum(by == l) for l in lab]) and got["p_above"] is None
        apart = fit.predict_groups(by, xb1, X=X1, groups=new, offset=off, row_weights=w, probs=probs, return_draws=True, combine_chains=False, seed=7)
        assert apart["average"].shape == (len(lab), 8, 2) and np.array_equal(combine_chains_f(apart["average"]), got["average"])
        # the levels split into several calls by a small limit: the same bits
        few = fit.predict_groups(by, xb1, X=X1, groups=new, offset=off, row_weights=w, probs=probs, return_draws=True, seed=7, level_bytes=8 * 16 * 3)
        for k in ("mean", "sd", "quantiles", "average", "weight", "count"):
            assert np.array_equal(few[k], got[k]), f"split into ranges of three levels: {k} differs"
        # by = the name of a grouping term
        term = fit.predict_groups("g.1", xb1, X=X1, groups=new, offset=off, statistic="sum", return_draws=True, seed=7)
        lev1 = np.asarray(d["g1"])[:m]
        assert np.array_equal(term["levels"], np.unique(lev1))
        np.testing.assert_allclose(term["average"], np.vstack([flat[lev1 == l].sum(axis=0) for l in np.unique(lev1)]), rtol=1e-11, atol=1e-12)
        # treatment=: the per-site average effect with P(effect > 0), against predict_contrast's rows
        eff = fit.predict_groups("g.1", xb1, X=X1, groups=new, offset=off, treatment=("x_bart", 9), threshold=0.0, return_draws=True, seed=7)
        xb0 = xb1.copy()
        t1 = xb1.copy()
        t1[:, 9], xb0[:, 9] = 1.0, 0.0
        d1 = combine_chains_f(fit.predict(x_bart=t1, X=X1, groups=new, offset=off, combine_chains=False, seed=7))
        d0 = combine_chains_f(fit.predict(x_bart=xb0, X=X1, groups=new, offset=off, combine_chains=False, seed=7))
        want = np.vstack([(d1 - d0)[lev1 == l].mean(axis=0) for l in np.unique(lev1)])
        np.testing.assert_allclose(eff["average"], want, rtol=1e-9, atol=1e-11)
        far = np.abs(want) > 1e-9
        assert np.array_equal((eff["average"] > 0.0)[far], (want > 0.0)[far]) and np.array_equal(eff["p_above"], (eff["average"] > 0.0).mean(axis=1))
        with pytest.raises(ValueError, match="'by' names the grouping term 'g.3'"):
            fit.predict_groups("g.3", xb1, groups=new)
        with pytest.raises(ValueError, match="does not hold one level"):
            fit.predict_groups(by, xb1, level_bytes=8)
    finally:
        fit.close()
