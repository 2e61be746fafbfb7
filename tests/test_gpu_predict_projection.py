"""s4b_predict_projection on the device (stan4bart_amd/csrc/readout_projection.inc: k_predict_values / k_contrast_values unchanged, k_proj_reduce<8 / 16 /
32>, k_proj_fold, k_proj_solve, k_level_rows and k_row_quantiles unchanged over the [(K + 1) x S] matrix) against numpy in long double on the full
matrix (tests/projection_cases.py: the model, the bounds, the designs).  The smallest shapes at which the reduction can go wrong: rows around one slab
of 128 and around 64, and 1 100 rows in 1, 2 and 9 chunks (the same bits); K = 1, 2, 8, 9, 16, 17, 32 (every template instance and its first
over-size); 1, 4 and 68 pooled draws (a second, partly filled block of lanes, pooled from samplers of different lengths); both routes, live and stored
samplers; one arm, two arms under the identity link (a BART column; no affected tree: route 0) and under the probit link; no weights, random weights, a
slab of zero weights, all weights zero; a duplicated column; the power-of-two column scaling and the swapped arms bit for bit; predict_groups and
predict_summary as cross-checks; the refusals before any launch; the device bytes; the Python interface.

Small Friedman chains, as tests/test_gpu_predict_groups.py builds them: n = 100, 5 trees, stored samplers of 1, 4, 9 and 64 draws; a binary chain
(11 trees; 5 and 13 draws) for link 1.  Measured on an MI355X, the largest |device - model| / bound of the module: coef 0.019, quantiles 0.012,
mean 0.011, r2 0.008, m2 0.002 (allowed: 4)."""
import struct

import numpy as np
import pytest

import contrast_cases as cc
import group_cases as gc
import pd_cases as pc
import projection_cases as pj
import quantile_cases as qc
import readout_cases as rc
import summary_cases as sc

pytestmark = pytest.mark.gpu
WORST = {}
PROBS = (0.025, 0.5, 0.975, 0.0, 1.0, 1.0 / 3.0)
FLOATS = ("coef", "r2", "mean", "m2", "quantiles", "p_above")


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
    c = Chain(hip_lib, rc._friedman(n=100, T=5, warmup=4, iter=4 + 64, ranef=False), rows=1100, steps=(1, 3, 5, 55))
    yield c
    c.close()
    print("predict_projection, largest |device - model| / bound of this module: " + ", ".join(f"{k} {r:.3g}" for k, r in WORST.items()))


@pytest.fixture(scope="module")
def binary(hip_lib):
    c = Chain(hip_lib, rc._binary(n=400, T=11, warmup=6, iter=19), rows=300, steps=(1, 1, 3, 8))
    yield c
    c.close()


_REF = {}


def _values(chain, lens, rows, arms=1, link=0, M=0, offset=False, col=None, dense0=False, swap=False, seed=0):
    """The keyword arguments of a pooled call over the first `rows` rows and the reference matrix x with its bound (computed once per key and left
    unchanged).  Every OCCURRENCE of a pooled sampler gets a coefficient table of its own.  Two arms: column `col` of the BART rows differs (None: no
    BART column), `dense0`: arm 0 has a dense part of its own; `swap` exchanges the arms."""
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


def _matrix(ref):
    return np.vstack([ref["coef"].astype(np.float64), ref["r2"].astype(np.float64)[None, :]])


def _case(chain, lens, rows, K, what, weights=None, probs=PROBS, threshold="midway", values=None, design=None, sampler=None, **call):
    """One pooled call through the C-ABI as it is (no column scaling) against the model.  threshold "midway": between two adjacent reference values."""
    kw, x, bx = _values(chain, lens, rows, **(values or {}))
    A = pj.design_matrix(rows, K, seed=K) if design is None else design
    if threshold == "midway":
        ref0, _ = pj.model(x, bx, A, weights)
        threshold = 0.0 if ref0["deficient"] else gc.midway(_matrix(ref0))
    ref, bd = pj.model(x, bx, A, weights, probs, threshold)
    if not ref["deficient"]:
        cond, worst = pj.check_inputs(ref, bd, what)
        _report(f"{what}: cond(G) = {cond:.3g}, largest bound of r2 = {worst:.3g}")
    got = (sampler or chain.stored[lens[0]]).predict_projection(design=A, weights=weights, probs=probs, threshold=threshold, scale_columns=False, **kw, **call)
    S, info = sum(lens), got["info"]
    assert got["draws_pooled"] == S and info["draws"] == S and info["columns"] == A.shape[1], info
    _note(pj.assert_projection(got, ref, bd, what, _report))
    return got, (ref, bd), dict(kw, design=A, weights=weights, probs=probs, threshold=threshold, scale_columns=False)


def _same_bits(a, b, what, keys=FLOATS + ("weight", "deficient")):
    for k in keys:
        assert (a.get(k) is None) == (b.get(k) is None), (what, k)
        if a.get(k) is not None:
            assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k} differs"


# ---- slab edges and chunking -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [63, 64, 65, 127, 128, 129, 1100])
def test_slab_edges_and_chunking(gauss, rows):
    S, K = 9, 3
    w = np.random.default_rng(rows).uniform(0.0, 2.0, rows)
    res = {}
    for name, C in (("C 128", 128), ("C 640", 640), ("one chunk", 0)):
        res[name], _, _ = _case(gauss, (S,), rows, K, f"{rows} rows, {name}", weights=w, values=dict(M=2, offset=True), scratch_bytes=C * 8 * S)
        info = res[name]["info"]
        want = min(rows, C) if C else rows
        assert info["rows_per_chunk"] == want and info["chunks"] == -(-rows // want) and info["deficient"] == 0, info
    _same_bits(res["C 128"], res["C 640"], f"{rows} rows: C 128 and C 640")
    _same_bits(res["C 128"], res["one chunk"], f"{rows} rows: C 128 and one chunk")
    if rows == 1100:
        assert [res[k]["info"]["chunks"] for k in ("C 128", "C 640", "one chunk")] == [9, 2, 1]
        assert res["C 128"]["info"]["launches"] == 9 * 5 + 3 and res["one chunk"]["info"]["launches"] == 5 + 3, res["C 128"]["info"]
        # a scratch limit that is no multiple of a slab's bytes rounds down to whole slabs
        odd, _, _ = _case(gauss, (S,), rows, K, "1100 rows, C 300 -> 256", weights=w, values=dict(M=2, offset=True), scratch_bytes=300 * 8 * S)
        assert odd["info"]["rows_per_chunk"] == 256
        _same_bits(res["one chunk"], odd, "C 256")


# ---- the design's columns --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 8, 9, 16, 17, 32])
def test_column_counts(gauss, K):
    rows, S = 300, 4
    w = np.random.default_rng(K).uniform(0.0, 2.0, rows)
    got, _, _ = _case(gauss, (S,), rows, K, f"K = {K}", weights=w, values=dict(M=1))
    assert got["coef"].shape == (K, S) and got["mean"].shape == (K + 1,) and got["quantiles"].shape == (len(PROBS), K + 1)
    few, _, _ = _case(gauss, (S,), rows, K, f"K = {K}, C 128", weights=w, values=dict(M=1), scratch_bytes=128 * 8 * S)
    _same_bits(got, few, f"K = {K}: one chunk and three")


# ---- draw counts -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [(1,), (4,), (64, 4), (4, 64)])
def test_draw_counts(gauss, lens):
    rows, K = 300, 5
    got, _, _ = _case(gauss, lens, rows, K, f"{sum(lens)} draws {lens}", weights=np.random.default_rng(7).uniform(0.5, 1.5, rows), values=dict(M=1), scratch_bytes=128 * 8 * sum(lens))
    if sum(lens) == 1:
        assert np.all(got["m2"] == 0.0) and np.array_equal(got["mean"][:K], got["coef"][:, 0]) and got["mean"][K] == got["r2"][0]
    if lens == (4, 64):          # (64, 4)'s pooled draw k is (4, 64)'s draw perm[k]
        other, _, _ = _case(gauss, (64, 4), rows, K, "68 draws (64, 4), no tables", threshold=None)
        mine, _, _ = _case(gauss, (4, 64), rows, K, "68 draws (4, 64), no tables", threshold=None)
        perm = np.r_[np.arange(4, 68), np.arange(4)]
        assert np.array_equal(mine["coef"][:, perm], other["coef"]) and np.array_equal(mine["r2"][perm], other["r2"]), "permuted peers: not the same values"
        assert np.array_equal(mine["quantiles"], other["quantiles"])


# ---- routes and samplers ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arms", [1, 2])
def test_routes_live_and_stored_two_calls(binary, arms):
    rows, S, K = 300, 13, 4
    values = dict(arms=arms, M=2, link=1, **(dict(col=binary.used_column(S), dense0=True) if arms == 2 else {}))
    w = np.random.default_rng(arms).uniform(0.0, 1.0, rows)
    res = {}
    for route in ("staged", "global"):
        res[route], _, call = _case(binary, (S,), rows, K, f"link 1, {arms} arm(s), {route}", weights=w, values=values, route=route)
        assert res[route]["info"]["route"] == (1 if route == "staged" else 2)
    _same_bits(res["staged"], res["global"], "the two routes")
    again = binary.stored[S].predict_projection(**call, route="global")
    _same_bits(res["global"], again, "two calls")
    live = binary.live.predict_projection(**call)
    _same_bits(res["staged"], live, "live and stored samplers")
    chunked = binary.live.predict_projection(**call, scratch_bytes=128 * 8 * S)
    _same_bits(res["staged"], chunked, "live, three chunks")


# ---- two arms under the identity link ---------------------------------------------------------------------------------------------------------------------
def test_two_arms_identity_link_and_no_affected_tree(gauss):
    rows, lens, K = 300, (9, 4), 4
    w = np.random.default_rng(2).uniform(0.0, 2.0, rows)
    col = gauss.used_column(9)
    a, _, _ = _case(gauss, lens, rows, K, "two arms, a BART column and a dense part", weights=w, values=dict(arms=2, M=2, col=col, dense0=True))
    assert a["info"]["route"] in (1, 2)
    b, _, call = _case(gauss, lens, rows, K, "two arms, a dense part only: no tree is walked", weights=w, values=dict(arms=2, M=2, dense0=True))
    assert b["info"]["route"] == 0, b["info"]
    c = gauss.stored[9].predict_projection(**call, scratch_bytes=128 * 8 * 13)
    _same_bits(b, c, "route 0: one chunk and three")


def test_swapped_arms_negate_bit_for_bit(gauss):
    """Swapping the arms negates every d bit for bit, so b and s, the coefficients and their mean; t, G, rss, tss and so r2 and every m2 are the same.
    Of the quantiles the probs 0 and 1 change places and the median of an ODD number of draws is one order statistic; an interpolated quantile is not
    the negative of the one formed from the other end (tests/test_gpu_predict_groups.py), so it is not compared.  9 pooled draws."""
    rows, lens, K = 300, (9,), 4
    w = np.random.default_rng(5).uniform(0.0, 1.0, rows)
    values = dict(arms=2, M=2, col=gauss.used_column(9), dense0=True)
    a, _, _ = _case(gauss, lens, rows, K, "two arms", weights=w, values=values, threshold=None)
    b, _, _ = _case(gauss, lens, rows, K, "two arms, swapped", weights=w, values=dict(values, swap=True), threshold=None)
    assert np.any(a["coef"] != 0.0)
    assert np.array_equal(b["coef"], -a["coef"]) and np.array_equal(b["mean"][:K], -a["mean"][:K]), "swapped arms do not negate bit for bit"
    assert np.array_equal(b["r2"], a["r2"]) and np.array_equal(b["m2"], a["m2"]) and b["mean"][K] == a["mean"][K]
    q0, q1, med = PROBS.index(0.0), PROBS.index(1.0), PROBS.index(0.5)
    assert np.array_equal(b["quantiles"][q0, :K], -a["quantiles"][q1, :K]) and np.array_equal(b["quantiles"][q1, :K], -a["quantiles"][q0, :K])
    assert np.array_equal(b["quantiles"][med, :K], -a["quantiles"][med, :K]) and np.array_equal(b["quantiles"][:, K], a["quantiles"][:, K])


# ---- weights ---------------------------------------------------------------------------------------------------------------------------------------------
def test_weights_none_a_slab_of_zeros_and_all_zero(gauss):
    rows, S, K = 400, 9, 4
    none, _, _ = _case(gauss, (S,), rows, K, "no weights", values=dict(M=1, offset=True))
    assert none["weight"] == float(rows)
    ones, _, _ = _case(gauss, (S,), rows, K, "weights 1", weights=np.ones(rows), values=dict(M=1, offset=True))
    _same_bits(none, ones, "no weights and weights 1")
    w = np.random.default_rng(3).uniform(0.5, 1.5, rows)
    w[128:256] = 0.0          # the second slab
    slab, _, call = _case(gauss, (S,), rows, K, "a slab of zero weights", weights=w, values=dict(M=1, offset=True))
    keep = np.r_[0:128, 256:rows]
    sub = {k: (None if v is None else np.asarray(v)[keep]) for k, v in call.items() if k in ("x_test", "offset", "dense", "design", "weights")}
    short = gauss.stored[S].predict_projection(**dict(call, **sub))
    for k in ("coef", "r2", "mean", "quantiles"):          # (the rows without weight add exact zeros: the same slabs of the rest, the same bits)
        assert np.array_equal(slab[k], short[k]), f"a slab of zero weights: {k} differs from the call without those rows"
    zero, _, _ = _case(gauss, (S,), rows, K, "all weights zero", weights=np.zeros(rows), values=dict(M=1, offset=True))
    assert zero["deficient"] == 2 and zero["weight"] == 0.0 and zero["info"]["launches"] == 0 and np.all(np.isnan(zero["coef"])) and np.all(np.isnan(zero["p_above"]))


# ---- deficient designs -----------------------------------------------------------------------------------------------------------------------------------
def test_duplicated_column_is_deficient(gauss):
    rows, S = 300, 9
    A = pj.design_matrix(rows, 4, seed=4)
    dup = np.column_stack([A, A[:, 2]])
    got, _, call = _case(gauss, (S,), rows, 5, "a duplicated column", design=dup, values=dict(M=1))
    assert got["deficient"] == 1 and got["info"]["deficient"] == 1 and got["info"]["launches"] > 0
    for k in FLOATS:
        assert np.all(np.isnan(got[k])), k
    zero = np.column_stack([A, np.zeros(rows)])
    assert gauss.stored[S].predict_projection(**dict(call, design=zero))["deficient"] == 1
    # the columns themselves are fine: the scaled binding answers the four of them
    ok = gauss.stored[S].predict_projection(**dict(call, design=A, scale_columns=True))
    assert ok["deficient"] == 0 and np.all(np.isfinite(ok["coef"]))


# ---- the power-of-two scaling ----------------------------------------------------------------------------------------------------------------------------
def test_a_column_times_eight_divides_its_coefficient_by_eight(gauss):
    rows, lens, K = 300, (9, 4), 9
    w = np.random.default_rng(8).uniform(0.0, 2.0, rows)
    a, _, call = _case(gauss, lens, rows, K, "K = 9", weights=w, values=dict(M=1), threshold=0.0)
    A8 = call["design"].copy()
    A8[:, 2] *= 8.0
    b = gauss.stored[9].predict_projection(**dict(call, design=A8))
    others = [j for j in range(K) if j != 2]
    assert np.array_equal(b["coef"][2], a["coef"][2] / 8.0) and np.array_equal(b["coef"][others], a["coef"][others]) and np.array_equal(b["r2"], a["r2"])
    assert b["mean"][2] == a["mean"][2] / 8.0 and b["m2"][2] == a["m2"][2] / 64.0 and np.array_equal(b["quantiles"][:, 2], a["quantiles"][:, 2] / 8.0)
    assert np.array_equal(b["mean"][others + [K]], a["mean"][others + [K]]) and np.array_equal(b["p_above"], a["p_above"])
    # the binding's own scaling gives the bits of the unscaled call back wherever a scale is 1, and the same values to rounding everywhere
    c = gauss.stored[9].predict_projection(**dict(call, design=A8, scale_columns=True))
    assert np.all(np.frexp(c["scale"])[0] == 0.5)
    np.testing.assert_allclose(c["coef"], b["coef"], rtol=1e-9, atol=1e-12)
    np.testing.assert_array_equal(c["p_above"], b["p_above"])


# ---- cross-checks against shipped calls -------------------------------------------------------------------------------------------------------------------
def test_indicator_columns_give_the_group_means(gauss):
    rows, lens = 300, (9, 4)
    level, L = gc.slab_labels(rows)
    full = [l for l in range(L) if np.any(level == l)]
    A = np.column_stack([(level == l).astype(np.float64) for l in full])
    w = np.random.default_rng(6).uniform(0.5, 1.5, rows)
    got, (ref, bd), call = _case(gauss, lens, rows, len(full), "indicator columns", weights=w, design=A, values=dict(M=2, offset=True), threshold=None)
    kw, x, bx = _values(gauss, lens, rows, M=2, offset=True)
    g = gauss.stored[9].predict_groups(level=level, n_levels=L, weights=w, statistic="mean", outputs=("draws",), presorted=True, **kw)
    gref, gbd = gc.model(x, bx, level, L, w, 1)
    r = gc.bound_ratio(got["coef"], g["draws"][full], bd["coef"] + gbd["draws"][full])
    print(f"indicator columns against predict_groups' means: {r:.3g} x the sum of both bounds")
    assert r <= gc.BOUND_FACTOR


def test_a_column_of_ones_gives_the_average(gauss):
    rows, lens = 1100, (9,)
    w = np.random.default_rng(9).uniform(0.0, 2.0, rows)
    got, (ref, bd), _ = _case(gauss, lens, rows, 1, "a column of ones", weights=w, design=np.ones((rows, 1)), values=dict(M=2, offset=True))
    kw, x, bx = _values(gauss, lens, rows, M=2, offset=True)
    wn = w / got["weight"]
    s = gauss.stored[9].predict_summary(weights=wn[None, :], **{k: v for k, v in kw.items() if k not in ("n_arms", "peers", "peer_dense_coef")})
    # predict_summary adds the same terms, weighted by w / W, in another order: summary_cases' bound of its average, and the rounding of w / W
    b2 = wn @ bx + (rows + 1) * gc.U * (wn @ np.abs(x))
    r = gc.bound_ratio(got["coef"][0], s["average"][:, 0], bd["coef"][0] + b2)
    print(f"a column of ones against predict_summary's average: {r:.3g} x the sum of both bounds")
    assert r <= gc.BOUND_FACTOR


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(gauss):
    rows, S = 300, 9
    x = np.asfortranarray(gauss.x[:rows])
    A = pj.design_matrix(rows, 4)
    live, smp = gauss.live, gauss.stored[S]

    def refused(match, **kw):
        before = live.get_counters()
        for s in (live, smp):
            args = dict(x_test=x, design=A, probs=(0.5,), scale_columns=False)
            args.update(kw)
            with pytest.raises(RuntimeError, match=match):
                s.predict_projection(**args)
            assert not any(s.projection_info.values()), s.projection_info
        assert np.array_equal(live.get_counters(), before), "a refused call launched something"

    def changed(i, j, v):
        out = A.copy()
        out[i, j] = v
        return out
    refused(r"predict_projection: n_columns must lie in \[1, 32\], not 33", design=pj.design_matrix(rows, 33))
    refused(r"predict_projection: n_columns must lie in \[1, 32\], not 0", design=np.zeros((rows, 0)))
    refused("predict_projection: 4 design columns, but only 3 rows", x_test=x[:3], design=A[:3])
    refused(r"predict_projection: design entry \(17, 2\) is not finite", design=changed(17, 2, np.nan))
    refused(r"predict_projection: design entry \(299, 0\) is not finite", design=changed(299, 0, -np.inf))
    for bad, name in ((-1.0, "-1"), (np.nan, "nan"), (np.inf, "inf")):
        w = np.ones(rows)
        w[17] = bad
        refused(f"predict_projection: weight {name}.* of row 17 is negative or not finite", weights=w)
    refused("predict_projection: n_arms must be 1 .* or 2 .*, not 3", n_arms=3)
    refused("predict_projection: n_arms = 1 takes no arm-0 pointer", x_test0=x)
    refused(r"predict_projection: tol must lie in \[0, 1\)", tol=1.0)
    refused(r"predict_projection: tol must lie in \[0, 1\)", tol=-1e-3)
    refused("predict_projection: prob 1.5.* outside", probs=(1.5,))
    ok = smp.predict_projection(x_test=x, design=A, probs=(0.5,), scale_columns=False)
    assert ok["info"]["launches"] == 2 + 3 + 3, ok["info"]          # G: reduce, fold; values, reduce, fold; solve, level rows, sort
    before = live.get_counters()
    live.predict_projection(x_test=x, design=A, scale_columns=False)
    assert live.get_counters()[2] == before[2] + 7


# ---- device bytes ----------------------------------------------------------------------------------------------------------------------------------------
def test_device_bytes(gauss):
    rows, S, T, K = 1100, 9, gauss.T, 9
    nodes = struct.unpack_from("<Q", gauss.stored[S].export_bart_state(), 28)[0]
    w = np.ones(rows)
    got, _, _ = _case(gauss, (S,), rows, K, "device bytes, one arm", weights=w, values=dict(M=2, offset=True), scratch_bytes=256 * 8 * S)
    C, Q = got["info"]["rows_per_chunk"], len(PROBS)
    assert C == 256
    value = qc.device_bytes_formula(gauss.P, rows, nodes, S, T, True, 2, 0, 0, C, 0) - 2 * 16          # (no quantiles per row, no probs there)
    want = pj.device_bytes_formula(value, rows, S, K, C, weights=True, p_above=True, Q=Q)
    print(f"device memory of the call: {got['info']['device_bytes']} bytes, the sum of DESIGN.md 5.13: {want}; the draws matrix would take {8 * rows * S}")
    assert got["info"]["device_bytes"] == want
    col = gauss.used_column(S)
    two, _, _ = _case(gauss, (S,), rows, 32, "device bytes, two arms", values=dict(arms=2, M=2, col=col, dense0=True), threshold=None, probs=(), scratch_bytes=256 * 8 * S)
    value = cc.device_bytes_formula(gauss.P, rows, nodes, S, T, 256, D=1, M=2, dense0=True, per_row=False)
    want = pj.device_bytes_formula(value, rows, S, 32, 256)
    assert two["info"]["device_bytes"] == want, (two["info"], want)


# ---- the Python interface --------------------------------------------------------------------------------------------------------------------------------
def test_whole_interface(hip_lib):
    """Stan4bartFit.predict_projection against numpy's least squares over fit.predict of the same seed: an intercept and two centred moderators on the
    fitted values and on the treatment effect, weights, names, chains pooled."""
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
        mods = np.column_stack([40.0 + 10.0 * g.normal(size=m), xb1[:, 0]])          # an "age" far from 0 and a BART predictor
        w = g.uniform(0.0, 2.0, m)
        probs = (0.025, 0.5, 0.975)

        def lstsq(flat):
            ctr = (w @ mods) / w.sum()
            A = np.column_stack([np.ones(m), mods - ctr])
            r = np.sqrt(w)[:, None]
            beta, *_ = np.linalg.lstsq(r * A, r * flat, rcond=None)
            res = flat - A @ beta
            r2 = 1.0 - (w @ (res * res)) / (w @ ((flat - (w @ flat) / w.sum()) ** 2))
            return ctr, beta, r2
        flat = combine_chains_f(fit.predict(x_bart=xb1, X=X1, groups=new, offset=off, combine_chains=False, seed=7))
        got = fit.predict_projection(mods, xb1, X=X1, groups=new, offset=off, row_weights=w, names=["age", "x1"], probs=probs, seed=7)
        ctr, beta, r2 = lstsq(flat)
        assert got["names"] == ["(Intercept)", "age", "x1"] and got["draws"] == 16 and got["deficient"] == 0 and got["coef"].shape == (3, 16)
        np.testing.assert_allclose(got["center"], np.r_[0.0, ctr], rtol=1e-14)
        np.testing.assert_allclose(got["coef"], beta, rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(got["coef"][0], (w @ flat) / w.sum(), rtol=1e-11, atol=1e-12)          # the intercept IS the weighted average
        np.testing.assert_allclose(got["r2"], r2, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(got["mean"], beta.mean(axis=1), rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(got["sd"], beta.std(axis=1, ddof=1), rtol=1e-7, atol=1e-11)
        np.testing.assert_allclose(got["quantiles"], np.quantile(beta, probs, axis=1), rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(got["r2_quantiles"], np.quantile(r2, probs), rtol=1e-8, atol=1e-10)
        assert np.isclose(got["r2_mean"], r2.mean()) and np.isclose(got["weight"], w.sum())
        far = np.abs(beta) > 1e-9
        assert np.array_equal((got["coef"] > 0.0)[far], (beta > 0.0)[far]) and np.array_equal(got["p_above"], (got["coef"] > 0.0).mean(axis=1))
        # the treatment effect's moderators
        eff = fit.predict_projection(mods, xb1, X=X1, groups=new, offset=off, treatment=("x_bart", 9), row_weights=w, threshold=0.5, seed=7)
        t1, t0 = xb1.copy(), xb1.copy()
        t1[:, 9], t0[:, 9] = 1.0, 0.0
        d1 = combine_chains_f(fit.predict(x_bart=t1, X=X1, groups=new, offset=off, combine_chains=False, seed=7))
        d0 = combine_chains_f(fit.predict(x_bart=t0, X=X1, groups=new, offset=off, combine_chains=False, seed=7))
        _, beta, r2 = lstsq(d1 - d0)
        np.testing.assert_allclose(eff["coef"], beta, rtol=1e-7, atol=1e-10)
        np.testing.assert_allclose(eff["r2"], r2, rtol=1e-6, atol=1e-9)
        assert np.array_equal(eff["p_above"], (eff["coef"] > 0.5).mean(axis=1))
        # without centring the far-off column makes the normal equations worse, not wrong; a copy of a column is refused an answer
        raw = fit.predict_projection(mods, xb1, X=X1, groups=new, offset=off, row_weights=w, center=False, seed=7)
        np.testing.assert_allclose(raw["coef"][1:], got["coef"][1:], rtol=1e-7, atol=1e-10)
        twice = fit.predict_projection(np.column_stack([mods, mods[:, 0]]), xb1, X=X1, groups=new, offset=off, seed=7)
        assert twice["deficient"] == 1 and np.all(np.isnan(twice["coef"])) and np.all(np.isnan(twice["mean"])) and np.isnan(twice["r2_mean"])
    finally:
        fit.close()
