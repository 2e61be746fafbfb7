"""s4b_predict_contrast on the device (stan4bart_amd/csrc/dev_contrast.inc: k_contrast_values<staged>, k_contrast_values<global>, k_contrast_reduce,
k_contrast_fold, and dev_quantile.inc's k_row_quantiles on the same scratch) against numpy in long double on the full matrices of both arms
(tests/contrast_cases.py: the model and the derived bounds).

The chains are those of tests/test_gpu_predict_quantiles.py (Friedman n = 400, T = 25, warmup 4, iter 17; binary n = 400, T = 11; stored samplers holding
1, 2, 5 and 13 draws; the hard rows of readout_cases).  Which BART columns the cases overwrite is settled from the kept trees, with pd_cases.affected, over both chains (the 25 trees of the Gaussian chain leave no draw with fewer than four affected trees, the 11 of the binary one do):
the cases together must contain a draw without an affected tree, a draw with the most the chain offers, and affected counts of 1, 3, 4 and 5 (the edges
of PS_WALK) — asserted, not assumed.  predict_bart of every sampler at both arms' rows and the leaf sums of the bounds are computed once per arm and
shared by the tests."""
import ctypes as C
import struct

import numpy as np
import pytest

import contrast_cases as cc
import pd_cases as pc
import readout_cases as rc
import summary_cases as sc
from conftest import make_sampler

pytestmark = pytest.mark.gpu
POOLS = {1: (1,), 2: (2,), 5: (5,), 13: (13,), 18: (5, 13), 65: (13,) * 5}          # pooled draws -> the stored samplers pooled, the first takes the call
PROBS = (0.025, 0.5, 0.975, 0.0, 1.0, 1.0 / 3.0)
ROWS = 1024 + 37          # the hard rows and more: two tiles of the value kernel, 17 slabs of the reduction with a last one of 37 rows


def _report(line):
    print(line)


class Chain(pc.Chain):
    """pd_cases.Chain (live sampler, stored samplers with their kept trees) over the rows of the quantile tests: the hard rows of the kept rules in front,
    new rows behind them; predict_bart and the leaf sums of every (sampler, arm) computed once."""

    def __init__(self, lib, args, steps=(1, 1, 3, 8), rows=2200, prefix="s4b_"):
        super().__init__(lib, prefix, args, steps=steps, rows=rows)
        try:
            hard, _ = rc.predict_case_rows("summary", args, dict(kept_trees=self.live.get_kept_trees()), 0)
            self.n_hard = len(hard)
            self.x = np.asfortranarray(np.vstack([hard, rc.new_rows(args.x_bart, max(1, rows - len(hard)), seed=3)]))
            self._bart, self._sums = {}, {}
        except Exception:
            self.close()
            raise

    def arms(self, rows, cols, partial=False, inside=None):
        """(arm 1, arm 0, key): arm 0 is arm 1 with the columns `cols` overwritten by training values of other rows (`partial`: in every third row
        only); column `inside` gets other raw values INSIDE the bins of the new rows (the next double: no cut lies between), which must not count."""
        x1 = np.asfortranarray(self.x[:rows])
        x0 = x1.copy()
        n = len(self.args.x_bart)
        for j in cols:
            other = self.args.x_bart[(np.arange(rows) * 7 + j + 1) % n, j]
            if partial:
                x0[::3, j] = other[::3]
            else:
                x0[:, j] = other
        if inside is not None and rows > self.n_hard:
            x0[self.n_hard:, inside] = np.nextafter(x1[self.n_hard:, inside], np.inf)
        return x1, x0, (rows, tuple(cols), partial, inside)

    def bart(self, S, key, x):
        if (S, key) not in self._bart:
            self._bart[S, key] = self.stored[S].predict_bart(x)
        return self._bart[S, key]

    def sums(self, S, key, x, cols):
        k = (S, key, tuple(cols))
        if k not in self._sums:
            self._sums[k] = cc.leaf_sums(self.trees[S], x, self.counts(S, cols, hit=True))
        return self._sums[k]

    def counts(self, S, cols, hit=False):
        h = self.hit(S, list(cols)) if len(cols) else np.zeros((S, self.T), dtype=bool)
        return h if hit else h.sum(axis=1)


@pytest.fixture(scope="module")
def gauss(hip_lib):
    c = Chain(hip_lib, rc._friedman(n=400, T=25, warmup=4, iter=17, ranef=False))
    yield c
    c.close()


@pytest.fixture(scope="module")
def binary(hip_lib):
    c = Chain(hip_lib, rc._binary(n=400, T=11, warmup=6, iter=19), rows=1300)
    yield c
    c.close()


def _inputs(chain, pool, rows, cols, M=0, E=0, offset=False, arm0=(), G=3, partial=False, inside=None, seed=0):
    """The arguments of a pooled call and what the model needs: (keyword arguments, parts, arm 1's row side, arm 0's, weights).  The row side is
    shared by the pool, every pooled sampler gets a coefficient table of its own; `arm0` names the parts arm 0 gets of its own: dense0, ell_value0,
    ell_index0 (arm 1's indices moved down one row: other padding), offset0."""
    x1, x0, key = chain.arms(rows, cols, partial, inside)
    shared = sc.linear_parts(rows, pool[0], M, E, seed=seed)
    tables = [shared] + [sc.linear_parts(rows, S, M, E, seed=seed + 100 + j) for j, S in enumerate(pool[1:])]
    off = float(chain.range[1] - chain.range[0]) * np.random.default_rng(seed).uniform(-1.0, 1.0, rows) if offset else None
    arm1 = dict(offset=off, dense=shared.get("dense"), ell_index=shared.get("ell_index"), ell_value=shared.get("ell_value"))
    other = sc.linear_parts(rows, 1, M, E, seed=seed + 50)
    a0 = dict(offset=off[::-1].copy() if "offset0" in arm0 else None, dense=other["dense"] if "dense0" in arm0 else None,
              ell_index=np.roll(shared["ell_index"], 1, axis=0) if "ell_index0" in arm0 else None, ell_value=other["ell_value"] if "ell_value0" in arm0 else None)
    w = sc.weight_vectors(rows, G, seed=seed) if G else None
    kw = dict(x_test=x1, x_test0=x0 if (len(cols) or inside is not None) else None, offset=off, offset0=a0["offset"], dense0=a0["dense"], ell_index0=a0["ell_index"],
              ell_value0=a0["ell_value"], weights=w, peers=[chain.stored[S] for S in pool[1:]], **shared)
    if M:
        kw["peer_dense_coef"] = [t["dense_coef"] for t in tables[1:]]
    if E:
        kw["peer_ell_coef"] = [t["ell_coef"] for t in tables[1:]]
    parts = []
    for S, t in zip(pool, tables):
        (F1, G1), (F0, G0) = chain.sums(S, key[:1], x1, cols), chain.sums(S, key, x0, cols)
        parts.append(dict(bart1=chain.bart(S, key[:1], x1), bart0=chain.bart(S, key, x0), F1=F1, F0=F0, G1=G1, G0=G0, n_affected=chain.counts(S, cols),
                          dense_coef=t.get("dense_coef"), ell_coef=t.get("ell_coef")))
    return kw, parts, arm1, a0, w


_REF = {}


def _launches(info, per_row, G, Q):
    return info["chunks"] * (1 + (1 if (per_row or G) else 0) + (1 if G else 0) + (1 if Q else 0))


def _case(chain, pool, rows, cols, what, probs=PROBS, link=0, M=0, E=0, offset=False, arm0=(), G=3, partial=False, inside=None, seed=0, **call):
    """One pooled call against the model; the reference of a case is computed once and shared by the routes."""
    kw, parts, arm1, a0, w = _inputs(chain, pool, rows, cols, M, E, offset, arm0, G, partial, inside, seed)
    got = chain.stored[pool[0]].predict_contrast(probs=probs, link=link, **kw, **call)
    S, info = sum(pool), got["info"]
    counts = np.concatenate([chain.counts(s, cols) for s in pool])
    assert got["draws"] == S and info["draws"] == S and info["differing_columns"] == len(cols), info
    assert info["largest_affected"] == counts.max() and info["total_affected"] == counts.sum(), (info, counts)
    assert info["launches"] == _launches(info, True, G, len(probs)), info
    key = (id(chain), pool, rows, tuple(cols), tuple(probs), link, M, E, offset, tuple(arm0), G, partial, inside, seed)
    if key not in _REF:
        _REF[key] = cc.model(parts, arm1, a0, chain.T, chain.range, chain.binary, link=link, weights=w, probs=probs)
    ref, bd = _REF[key]
    cc.assert_contrast(got, ref, bd, what, _report)
    return got, (ref, bd), kw


def _same_bits(a, b, keys=("mean", "m2", "average", "quantiles")):
    return all(np.array_equal(a[k], b[k]) for k in keys)


# ---- differing columns -----------------------------------------------------------------------------------------------------------------------------------
def _column_cases(chains, S):
    """(chain, column set) cases, singles and pairs, chosen from the kept trees so that together their per-draw affected counts contain 0, 1, 3, 4, 5 and
    the largest count any single or pair of any of the chains reaches; at least one single and one pair."""
    cand = [(ch, c) for ch in chains for c in [(j,) for j in range(ch.P)] + [(i, j) for i in range(ch.P) for j in range(i + 1, ch.P)]]
    counts = {(id(ch), c): ch.counts(S, c) for ch, c in cand}
    seen = lambda case: set(counts[id(case[0]), case[1]].tolist())
    top = max(cand, key=lambda case: max(seen(case)))
    chosen, wanted = [top], {0, 1, 3, 4, 5} - seen(top)
    while wanted:
        best = max(cand, key=lambda case: (len(wanted & seen(case)), -len(case[1])))
        assert wanted & seen(best), f"no column set of these chains has a draw with {sorted(wanted)} affected trees: the cases do not cover the walk's edges"
        chosen.append(best)
        wanted -= seen(best)
    for n in (1, 2):
        if not any(len(c) == n for _, c in chosen):
            chosen.append(next(case for case in cand if len(case[1]) == n and max(seen(case)) > 0))
    return chosen, counts, max(seen(top))


def test_differing_columns_cover_the_edges_of_the_walk(gauss, binary):
    S, pool = 13, POOLS[13]
    chosen, counts, most = _column_cases((gauss, binary), S)
    seen = set()
    for n, (chain, cols) in enumerate(chosen):
        name = "binary" if chain is binary else "gauss"
        inside = next(j for j in range(chain.P) if j not in cols)
        res = {}
        for route in ("staged", "global"):
            res[route], *_ = _case(chain, pool, ROWS, cols, f"{name}, columns {cols} {route}", partial=(n % 2 == 1), inside=inside, seed=n, route=route)
            assert res[route]["info"]["route"] == (1 if route == "staged" else 2)
        assert _same_bits(res["staged"], res["global"]), "the two routes differ"
        assert res["staged"]["info"]["largest_affected"] == counts[id(chain), cols].max()
        seen |= set(counts[id(chain), cols].tolist())
    print(f"column sets {[(('binary' if ch is binary else 'gauss'), c) for ch, c in chosen]}: affected counts per draw {sorted(seen)}, the most {most}")
    assert {0, 1, 3, 4, 5, most} <= seen and {len(c) for _, c in chosen} == {1, 2}
    # D = 0: arm 0 given, other raw values inside the bins only — no column differs, no tree is walked under link 0
    got, *_ = _case(gauss, pool, ROWS, (), "raw values inside the bins", inside=0)
    assert got["info"]["route"] == 0 and got["info"]["total_affected"] == 0 and not got["mean"].any() and not got["quantiles"].any() and not got["average"].any()


# ---- links and linear parts ------------------------------------------------------------------------------------------------------------------------------
def _used_column(chain, S):
    return max(range(chain.P), key=lambda j: int(chain.counts(S, (j,)).sum()))


@pytest.mark.parametrize("arm0", [(), ("dense0",), ("ell_value0",), ("ell_index0",), ("offset0",), ("dense0", "ell_value0", "ell_index0", "offset0")],
                         ids=lambda a: "+".join(a) or "shared")
def test_links_and_linear_parts(gauss, binary, arm0):
    assert binary.args.is_binary and not gauss.args.is_binary
    for chain, name in ((binary, "binary"), (gauss, "gauss")):
        cols = (_used_column(chain, 13),)
        for link in (1, 0):
            got, _, kw = _case(chain, POOLS[18], 300, cols, f"{name} link {link} arm 0: {arm0}", link=link, M=17, E=3, offset=True, arm0=arm0, seed=link)
            if "ell_index0" in arm0:
                ix, ix0 = kw["ell_index"], kw["ell_index0"]
                assert ((ix == -1) != (ix0 == -1)).any() and (ix == -1).any() and len({int(n) for n in (ix >= 0).sum(axis=1)}) > 1, "the padding is not ragged or not another one"
            if link:
                assert np.all(np.abs(got["quantiles"]) <= 1) and np.all(np.abs(got["mean"]) <= 1)


def test_linear_parts_that_differ_while_no_column_does(gauss):
    for arm0 in (("dense0",), ("dense0", "ell_value0", "ell_index0", "offset0")):
        for link in (0, 1):
            got, (ref, bd), kw = _case(gauss, POOLS[18], 300, (), f"D 0, link {link}, arm 0: {arm0}", link=link, M=3, E=2, offset=True, arm0=arm0, seed=7)
            assert got["info"]["differing_columns"] == 0 and got["info"]["route"] == (0 if not link else 1) and got["mean"].any()
    # link 0, dense0 only: d is the linear difference, whatever the trees — the model's bound then holds no tree term at all
    got, (ref, bd), kw = _case(gauss, POOLS[13], 300, (), "D 0, dense0 only", M=3, arm0=("dense0",), probs=(0.0, 1.0), seed=8)
    want = ((kw["dense"].astype(cc.LD) - kw["dense0"].astype(cc.LD)) @ kw["dense_coef"].T.astype(cc.LD))
    assert cc.bound_ratio(ref["d"], want.astype(np.float64), bd["d"] + cc.U * np.abs(ref["d"])) <= cc.BOUND_FACTOR
    assert np.all(bd["d"] <= 8 * 3 * cc.U * (np.abs(kw["dense"]) + np.abs(kw["dense0"])).sum(axis=1).max() * np.abs(kw["dense_coef"]).max())


# ---- pools and routes ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", sorted(POOLS))
def test_pooled_draw_counts_against_the_model_on_both_routes(gauss, S):
    pool, cols = POOLS[S], (_used_column(gauss, 13),)
    res = {}
    for route in ("staged", "global"):
        res[route], (ref, bd), kw = _case(gauss, pool, ROWS, cols, f"S {S} {route}", M=2, E=2, offset=True, arm0=("dense0", "ell_value0"), seed=S, route=route)
        info = res[route]["info"]
        assert info["route"] == (1 if route == "staged" else 2) and info["rows_per_chunk"] == ROWS and info["chunks"] == 1
    assert _same_bits(res["staged"], res["global"]), "the two routes differ"
    got = res["staged"]
    assert got["average"].shape == (S, 3) and got["quantiles"].shape == (len(PROBS), ROWS)
    if S == 1:
        assert not got["m2"].any(), "one draw: m2 is exactly 0"
        assert np.array_equal(got["quantiles"], np.repeat(got["mean"][None, :], len(PROBS), axis=0))
    if len(pool) > 1:          # every peer's own table reached its draws: the model with the first table for all is another answer
        _, parts, arm1, a0, w = _inputs(gauss, pool, ROWS, cols, 2, 2, True, ("dense0", "ell_value0"), 3, seed=S)
        same = [dict(p, dense_coef=np.resize(parts[0]["dense_coef"], p["dense_coef"].shape), ell_coef=np.resize(parts[0]["ell_coef"], p["ell_coef"].shape)) for p in parts]
        other, obd = cc.model(same, arm1, a0, gauss.T, gauss.range, gauss.binary, weights=w, probs=PROBS)
        assert cc.bound_ratio(got["quantiles"], other["quantiles"], obd["quantiles"]) > 1e6, "the peers' coefficient tables do not matter: the case tests no per-peer table"


# ---- bit-exact anchors -----------------------------------------------------------------------------------------------------------------------------------
def test_identical_arms_are_exactly_zero(gauss, binary):
    for chain in (gauss, binary):
        for link in (0, 1):
            kw, *_ = _inputs(chain, POOLS[18], 300, (), M=2, E=2, offset=True, seed=link)
            for x0 in (None, kw["x_test"].copy()):
                got = chain.stored[5].predict_contrast(probs=PROBS, link=link, **dict(kw, x_test0=x0))
                for key in ("mean", "m2", "average", "quantiles"):
                    assert got[key].size and not got[key].any() and np.all(np.isfinite(got[key])), (key, link)
                info = got["info"]
                assert info["differing_columns"] == 0 and info["total_affected"] == 0 and info["route"] == (1 if link else 0), info
                assert info["launches"] == 4 and info["draws"] == 18


def test_swapped_arms_negate_bit_for_bit(gauss, binary):
    probs = (0.0, 1.0, 0.5, 0.25, 0.75)          # 13 draws: h = p * 12 is an integer, and so is that of 1 - p
    mirror = (1, 0, 2, 4, 3)
    for chain in (gauss, binary):
        cols = (_used_column(chain, 13),)
        for link in (0, 1):
            for route in ("staged", "global"):
                a, _, kw = _case(chain, POOLS[13], 700, cols, f"swap, link {link} {route}", probs=probs, link=link, M=3, E=2, offset=True,
                                 arm0=("dense0", "ell_value0", "ell_index0", "offset0"), seed=link, route=route)
                swapped = dict(kw, x_test=kw["x_test0"], x_test0=kw["x_test"], dense=kw["dense0"], dense0=kw["dense"], offset=kw["offset0"], offset0=kw["offset"],
                               ell_index=kw["ell_index0"], ell_index0=kw["ell_index"], ell_value=kw["ell_value0"], ell_value0=kw["ell_value"])
                b = chain.stored[13].predict_contrast(probs=probs, link=link, route=route, **swapped)
                assert a["mean"].any() and np.array_equal(b["mean"], -a["mean"]) and np.array_equal(b["average"], -a["average"]), (link, route)
                assert np.array_equal(b["m2"], a["m2"]), (link, route)
                for j, m in enumerate(mirror):
                    assert np.array_equal(b["quantiles"][j], -a["quantiles"][m]), (link, route, probs[j])


def test_pooling_order_self_pooling_and_live_samplers(gauss):
    rows, cols = 500, (_used_column(gauss, 13),)
    a, _, kw = _case(gauss, (2, 5, 13), rows, cols, "pool 2 + 5 + 13", M=1, E=2, offset=True, arm0=("dense0",), seed=3)
    peers, pd, pe = kw["peers"], kw["peer_dense_coef"], kw["peer_ell_coef"]
    rest = {k: v for k, v in kw.items() if k not in ("peers", "peer_dense_coef", "peer_ell_coef", "dense_coef", "ell_coef")}
    b = gauss.stored[13].predict_contrast(probs=PROBS, peers=[gauss.stored[2], peers[0]], dense_coef=pd[1], ell_coef=pe[1],
                                          peer_dense_coef=[kw["dense_coef"], pd[0]], peer_ell_coef=[kw["ell_coef"], pe[0]], **rest)
    assert b["draws"] == 20 and np.array_equal(a["quantiles"], b["quantiles"]), "permuting the pool changes the quantile bits"
    assert np.array_equal(b["average"][13:15], a["average"][:2]) and np.array_equal(b["average"][:13], a["average"][7:]), "average is draw-major in pooling order"
    # the live sampler holds the kept trees of stored[13]
    c = gauss.live.predict_contrast(probs=PROBS, peers=[gauss.stored[2], peers[0]], dense_coef=pd[1], ell_coef=pe[1],
                                    peer_dense_coef=[kw["dense_coef"], pd[0]], peer_ell_coef=[kw["ell_coef"], pe[0]], **rest)
    assert _same_bits(b, c) and c["info"] == b["info"]
    # a sampler pooled with itself: all ties — minimum, median and maximum are those of the sampler alone
    plain = {k: v for k, v in rest.items() if k in ("x_test", "x_test0")}
    for S in (5, 13):
        alone = gauss.stored[S].predict_contrast(probs=[0.0, 0.5, 1.0], **plain)
        for times in (2, 3):
            again = gauss.stored[S].predict_contrast(probs=[0.0, 0.5, 1.0], peers=[gauss.stored[S]] * (times - 1), **plain)
            assert again["draws"] == times * S and np.array_equal(again["quantiles"], alone["quantiles"]), (S, times)


# ---- against the existing kernels ------------------------------------------------------------------------------------------------------------------------
def test_mean_and_average_against_predict_summary(gauss):
    S, rows, cols = 13, 700, (_used_column(gauss, 13),)
    for link in (0, 1):
        got, (ref, bd), kw = _case(gauss, POOLS[S], rows, cols, f"against predict_summary, link {link}", link=link, M=2, E=2, offset=True, arm0=("dense0", "offset0"), seed=4)
        smp, w = gauss.stored[S], kw["weights"]
        lin = {k: kw[k] for k in ("dense_coef", "ell_index", "ell_value", "ell_coef")}
        one = smp.predict_summary(kw["x_test"], offset=kw["offset"], dense=kw["dense"], link=link, **lin)
        zero = smp.predict_summary(kw["x_test0"], offset=kw["offset0"], dense=kw["dense0"], link=link, **lin)
        key1, key0 = (rows,), (rows, cols, False, None)
        _, b1 = sc.model(gauss.bart(S, key1, kw["x_test"]), kw["offset"], kw["dense"], link=link, **lin)
        _, b0 = sc.model(gauss.bart(S, key0, kw["x_test0"]), kw["offset0"], kw["dense0"], link=link, **lin)
        r = cc.bound_ratio(got["mean"], one["mean"] - zero["mean"], bd["mean"] + b1["mean"] + b0["mean"] + cc.U * np.abs(got["mean"]))
        stacked = dict(offset=np.r_[kw["offset"], kw["offset0"]], dense=np.vstack([kw["dense"], kw["dense0"]]), ell_index=np.vstack([kw["ell_index"]] * 2),
                       ell_value=np.vstack([kw["ell_value"]] * 2), dense_coef=kw["dense_coef"], ell_coef=kw["ell_coef"])
        xs, ws = np.asfortranarray(np.vstack([kw["x_test"], kw["x_test0"]])), np.hstack([w, -w])
        both = smp.predict_summary(xs, weights=ws, link=link, **stacked)
        _, bs = sc.model(np.vstack([gauss.bart(S, key1, kw["x_test"]), gauss.bart(S, key0, kw["x_test0"])]), link=link, weights=ws, **stacked)
        ra = cc.bound_ratio(got["average"], both["average"], bd["average"] + bs["average"])
        print(f"link {link}: |contrast - difference of two predict_summary calls| / (sum of the bounds): mean {r:.3g}, average {ra:.3g}")
        assert r <= cc.BOUND_FACTOR and ra <= cc.BOUND_FACTOR


# ---- chunks, output selection, determinism ---------------------------------------------------------------------------------------------------------------
def test_chunks_of_rows(gauss):
    pool, S, cols = POOLS[18], 18, (_used_column(gauss, 13),)
    for rows, Cr, chunks in ((130, 64, 3), (2 * 1024 + 1, 1024 + 64, 2)):
        whole, (ref, bd), kw = _case(gauss, pool, rows, cols, f"{rows} rows in one chunk", M=1, E=1, offset=True, arm0=("dense0",), seed=rows)
        assert whole["info"]["chunks"] == 1 and whole["info"]["rows_per_chunk"] == rows and whole["info"]["launches"] == 4
        for route in ("staged", "global"):
            got = gauss.stored[pool[0]].predict_contrast(probs=PROBS, scratch_bytes=8 * S * Cr + 8 * S * 63, route=route, **kw)          # (rounded down to 64 rows)
            info = got["info"]
            assert (info["rows_per_chunk"], info["chunks"], info["launches"]) == (Cr, chunks, 4 * chunks), info
            assert rows - (chunks - 1) * Cr in (2, 961) and _same_bits(got, whole, ("mean", "m2", "quantiles")), f"{rows} rows in chunks of {Cr}: other bits"
            cc.assert_contrast(got, ref, bd, f"{rows} rows in chunks of {Cr}, {route}", _report, keys=("average",))


def test_output_selection_and_its_launches(gauss):
    rows, cols = 300, (_used_column(gauss, 13),)
    kw, *_ = _inputs(gauss, POOLS[18], rows, cols, M=1, offset=True, arm0=("dense0",), seed=2)
    smp = gauss.stored[5]
    full = smp.predict_contrast(probs=PROBS, **kw)
    for name, probs, w, per_row, launches in (("only mean and m2", (), None, True, 2), ("no probs", (), kw["weights"], True, 3), ("no weights", PROBS, None, True, 3),
                                               ("probs alone", PROBS, None, False, 2), ("weights alone", (), kw["weights"], False, 3),
                                               ("weights and probs", PROBS, kw["weights"], False, 4)):
        got = smp.predict_contrast(probs=probs, per_row=per_row, **dict(kw, weights=w))
        assert got["info"]["launches"] == launches == _launches(got["info"], per_row, w is not None, len(probs)), (name, got["info"])
        assert (got["mean"] is None) == (not per_row) and got["average"].shape == (18, 3 if w is not None else 0) and got["quantiles"].shape == (len(probs), rows)
        assert all(np.array_equal(got[k], full[k]) for k in ("mean", "m2", "average", "quantiles") if got[k] is not None and got[k].size), name
    assert full["info"]["launches"] == 4
    with pytest.raises(RuntimeError, match="nothing asked for"):
        smp.predict_contrast(probs=(), per_row=False, **dict(kw, weights=None))
    assert not any(smp.contrast_info.values())


def test_same_call_twice_is_bit_identical(gauss):
    cols = (_used_column(gauss, 13),)
    for route in ("staged", "global"):
        a, _, kw = _case(gauss, POOLS[65], 2 * 1024 + 1, cols, f"determinism {route}", link=1, M=3, E=3, offset=True, arm0=("dense0", "ell_index0"), route=route,
                         scratch_bytes=8 * 65 * 1088)
        b = gauss.stored[13].predict_contrast(probs=PROBS, link=1, route=route, scratch_bytes=8 * 65 * 1088, **kw)
        assert a["info"]["chunks"] == 2 and _same_bits(a, b), route


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(hip_lib, gauss, binary):
    rows, S = 50, 13
    x = np.asfortranarray(gauss.x[:rows])
    live = gauss.live
    parts = sc.linear_parts(rows, S, 1, 2)
    peer = sc.linear_parts(rows, 5, 1, 2, seed=1)

    def arm0(*cols):
        x0 = x.copy()
        for j in cols:
            x0[:, j] = gauss.args.x_bart[(np.arange(rows) * 7 + j + 1) % 400, j]
        return x0

    def refused(match, samplers=None, x0=None, **kw):
        before = live.get_counters()
        for smp in samplers or (live, gauss.stored[S]):
            with pytest.raises(RuntimeError, match=match):
                smp.predict_contrast(x, arm0(0) if x0 is None else x0, **{"probs": (0.5,), **kw})
            assert smp.contrast_info["launches"] == 0 and not any(smp.contrast_info.values())
        assert np.array_equal(live.get_counters(), before), "a refused call launched something"
    refused(r"predict_contrast: the arms differ in 3 BART columns \(1, 4, 6\), at most 2 are supported", x0=arm0(6, 1, 4))
    refused("predict_contrast: offset0 given, but arm 1 has no offset", offset0=np.zeros(rows))
    refused("predict_contrast: dense0 given, but arm 1 has no dense part", dense0=np.zeros((rows, 2)))
    refused("predict_contrast: ell_index0 / ell_value0 given, but arm 1 has no ELL part", ell_value0=np.zeros((rows, 2)))
    refused("predict_contrast: ell_index0 / ell_value0 given, but arm 1 has no ELL part", ell_index0=np.zeros((rows, 2), dtype=np.int32))
    refused(r"predict_contrast: ell_index0 7 outside \[-1, 7\)", ell_index0=np.full((rows, 2), 7, dtype=np.int32), **parts)
    nan = arm0(0)
    nan[rows - 1, gauss.P - 1] = np.nan
    refused("predict_contrast: x_test0 holds a NaN", x0=nan)
    refused("predict_contrast: between 0 and 8 weight vectors, not 9", weights=np.ones((9, rows)))
    refused("predict_contrast: between 0 and 16 probs per call, not 17", probs=np.linspace(0, 1, 17))
    refused(r"predict_contrast: prob -0\.1\d* outside \[0, 1\]", probs=(0.5, -0.1))
    refused(r"predict_contrast: prob 1\.5\d* outside \[0, 1\]", probs=(1.5,))
    refused(r"predict_contrast: prob -?nan outside \[0, 1\]", probs=(0.1, np.nan, 0.9))
    refused("predict_contrast: link must be 0", link=2)
    refused("predict_contrast: negative scratch_bytes", scratch_bytes=-1)
    # every peer refusal of predict_quantiles, under this entry's name
    assert binary.args.n_trees != gauss.args.n_trees
    refused("predict_contrast: peer 1 has 11 trees per draw, the sampler 25", peers=[gauss.stored[5], binary.stored[5]])
    refused("predict_contrast: n_dense > 0 needs peer_dense_coef", peers=[gauss.stored[5]], dense=parts["dense"], dense_coef=parts["dense_coef"])
    refused("predict_contrast: n_ell > 0 needs peer_ell_coef", peers=[gauss.stored[5]], peer_dense_coef=[peer["dense_coef"]], **parts)
    other = make_sampler(hip_lib, "s4b_", rc._friedman(n=410, T=25, warmup=2, iter=3, ranef=False))
    fresh = make_sampler(hip_lib, "s4b_", gauss.args)          # keep_trees, but no sampling run yet
    try:
        other.run(2, True)
        other.disengage_adaptation()
        other.run(1, False)
        refused(r"predict_contrast: peer 0 has other cut points of predictor \d+", peers=[other])
        refused("predict_contrast: peer 1 holds no kept draws", peers=[gauss.stored[5], fresh])
        refused("predict_contrast: the sampler holds no kept draws", samplers=(fresh,))
    finally:
        other.free()
        fresh.free()
    before = live.get_counters()
    with pytest.raises(RuntimeError, match="predict_contrast: 16393 pooled draws, at most 16384"):
        live.predict_contrast(x[:3], arm0(0)[:3], probs=[0.5], peers=[gauss.stored[13]] * 1260)
    assert not any(live.contrast_info.values()) and np.array_equal(live.get_counters(), before)
    # NULL peers in the structure, a per-row output given by halves (the Python method offers neither: the structures are filled here)
    from stan4bart_amd.abi import ContrastIn, ContrastOut, Sampler
    rows_in, keep, _, _ = Sampler._summary_in(S, x, None, None, None, None, None, None, 0, None, "auto", 0, 0)
    buf = np.zeros(rows)
    dp = C.POINTER(C.c_double)
    for arg, out, msg in ((ContrastIn(rows=rows_in, n_peers=1), ContrastOut(mean=buf.ctypes.data_as(dp), m2=buf.ctypes.data_as(dp)), "n_peers > 0 needs peers"),
                          (ContrastIn(rows=rows_in), ContrastOut(mean=buf.ctypes.data_as(dp)), "mean and m2 are given together or not at all")):
        assert hip_lib.s4b_predict_contrast(live._h, C.byref(arg), C.byref(out)) == 1
        assert msg in hip_lib.s4b_last_error().decode() and not any(out.info) and np.array_equal(live.get_counters(), before)
    ok = live.predict_contrast(x, arm0(0), probs=[0.5], peers=[gauss.stored[5]], peer_dense_coef=[peer["dense_coef"]], peer_ell_coef=[peer["ell_coef"]], **parts)
    assert ok["info"]["launches"] == 3 and live.get_counters()[2] == before[2] + 3 and ok["draws"] == 18


# ---- the whole interface ---------------------------------------------------------------------------------------------------------------------------------
def test_whole_interface_live_and_stored(hip_lib):
    """Stan4bartFit.predict_contrast against the model over fit.predict(arm 1) - fit.predict(arm 0) of the same seed and against np.quantile / np.std:
    two chains, the treatment among the BART predictors and the fixed effects and as a random slope, unseen levels; explicit arms and `treatment=`;
    live samplers and stored ones."""
    from stan4bart_amd import GroupTerm, generate_friedman_data
    from stan4bart_amd.abi import Sampler
    from stan4bart_amd.generics import combine_chains_f, stan4bart
    d = generate_friedman_data(120, ranef=True, causal=True, p=10)
    x, z = d["x"], np.asarray(d["z"], dtype=np.float64)
    xb, X = np.column_stack([x[:, [j for j in range(10) if j != 3]], z]), np.column_stack([x[:, 3], z])
    groups = [GroupTerm(d["g1"], z, "g.1"), GroupTerm(d["g2"], None, "g.2")]
    fit = stan4bart(d["y"], xb, X=X, groups=groups, chains=2, seed=99, iter=14, warmup=6, bart_args={"n.trees": 9, "keepTrees": True},
                    make_sampler=lambda a, st: Sampler(hip_lib, "s4b_", a, st))
    try:
        m = 45
        g = np.random.default_rng(11)
        lev1 = np.asarray(d["g1"])[:m].copy()
        lev1[::4] = 6 + (np.arange(len(lev1[::4])) % 2)          # g.1 has five levels: 6 and 7 are unseen
        xb1 = rc.new_rows(xb, m, seed=4)
        xb0 = xb1.copy()
        xb1[:, 9], xb0[:, 9] = 1.0, 0.0
        X1 = X[:m] + g.normal(size=(m, 2))
        X0 = X1.copy()
        X1[:, 1], X0[:, 1] = 1.0, 0.0
        off = g.normal(size=m)
        new1 = [GroupTerm(lev1, np.ones(m), "g.1"), GroupTerm(np.asarray(d["g2"])[:m], None, "g.2")]
        new0 = [GroupTerm(lev1, np.zeros(m), "g.1"), GroupTerm(np.asarray(d["g2"])[:m], None, "g.2")]
        full1 = fit.predict(x_bart=xb1, X=X1, groups=new1, offset=off, combine_chains=False, seed=7)          # [rows, iter, chain]
        full0 = fit.predict(x_bart=xb0, X=X0, groups=new0, offset=off, combine_chains=False, seed=7)
        flat = combine_chains_f(full1) - combine_chains_f(full0)
        assert flat.shape == (m, 16) and flat.any()
        # the model over the builder's own stacked table
        stacked = [GroupTerm(np.r_[lev1, lev1], np.r_[np.ones(m), np.zeros(m)], "g.1"), GroupTerm(np.tile(np.asarray(d["g2"])[:m], 2), None, "g.2")]
        ix, val, coef = fit._ell_random(stacked, True, np.random.default_rng(7))
        assert ix.max() >= fit.stan[fit._rows("b.")].shape[0], "no unseen level reached the table"
        beta = fit.stan[fit._rows("beta.")]
        probs = (0.025, 0.5, 0.975, 0.2)
        w = np.vstack([np.full(m, 1.0 / m), (np.arange(m) % 2) / (m // 2)])
        trees = [s.get_kept_trees() for s in fit.samplers]
        parts = []
        for c, s in enumerate(fit.samplers):
            hit = pc.affected(trees[c], [9], 8, 9)
            (F1, G1), (F0, G0) = cc.leaf_sums(trees[c], xb1, hit), cc.leaf_sums(trees[c], xb0, hit)
            parts.append(dict(bart1=s.predict_bart(xb1), bart0=s.predict_bart(xb0), F1=F1, F0=F0, G1=G1, G0=G0, n_affected=hit.sum(axis=1),
                              dense_coef=beta[:, :, c].T, ell_coef=coef[c]))
        arm1 = dict(offset=off, dense=X1 - fit.X_means, ell_index=ix[:m], ell_value=val[:m])
        a0 = dict(dense=X0 - fit.X_means, ell_index=ix[m:], ell_value=val[m:])
        ref, bd = cc.model(parts, arm1, a0, 9, fit.samplers[0].get_bart_data_range(), False, weights=w, probs=probs)
        np.testing.assert_allclose(ref["d"], flat, rtol=1e-9, atol=1e-11)          # fit.predict and the model over the ELL table describe the same draws

        def check(what):
            got = fit.predict_contrast(xb1, xb0, X=X1, X0=X0, groups=new1, groups0=new0, offset=off, row_weights=w, probs=probs, seed=7)
            assert got["draws"] == 16 and got["quantiles"].shape == (4, m) and got["average"].shape == (2, 16) and np.array_equal(got["probs"], probs)
            ratios = dict(mean=cc.bound_ratio(got["mean"], ref["mean"], bd["mean"]), m2=cc.bound_ratio(got["sd"] ** 2 * 15, ref["m2"], bd["m2"] + 4 * cc.U * ref["m2"]),
                          average=cc.bound_ratio(got["average"], ref["average"].T, bd["average"].T), quantiles=cc.bound_ratio(got["quantiles"], ref["quantiles"], bd["quantiles"]))
            print(f"whole interface, {what}: max |device - model| / bound: " + ", ".join(f"{k} {r:.3g}" for k, r in ratios.items()))
            assert max(ratios.values()) <= cc.BOUND_FACTOR, ratios
            np.testing.assert_allclose(got["quantiles"], np.quantile(flat, probs, axis=1), rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(got["sd"], np.std(flat, axis=1, ddof=1), rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(got["mean"], flat.mean(axis=1), rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(got["average"], w @ flat, rtol=1e-9, atol=1e-12)
            apart = fit.predict_contrast(xb1, xb0, X=X1, X0=X0, groups=new1, groups0=new0, offset=off, row_weights=w, probs=probs, seed=7, combine_chains=False)
            assert apart["average"].shape == (2, 8, 2) and np.array_equal(combine_chains_f(apart["average"]), got["average"])
            # `treatment=` against the same arms given explicitly: the same bits
            t = fit.predict_contrast(xb1, X=X1, groups=new1, offset=off, treatment=("x_bart", 9), seed=7)
            e = fit.predict_contrast(xb1, xb0, X=X1, groups=new1, offset=off, seed=7)
            assert all(np.array_equal(t[k], e[k]) for k in ("mean", "sd", "average", "quantiles")) and t["mean"].any()
            bart = fit.predict_contrast(xb1, xb0, type="indiv.bart")
            np.testing.assert_allclose(bart["mean"], np.concatenate([p["bart1"] - p["bart0"] for p in parts], axis=1).mean(axis=1), rtol=1e-9, atol=1e-12)
            return got, t
        a, ta = check("live samplers")
        fit.attach_stored_samplers(fit.export_bart_states(), lib=hip_lib)
        b, tb = check("stored samplers")
        assert all(np.array_equal(a[k], b[k]) and np.array_equal(ta[k], tb[k]) for k in ("mean", "sd", "average", "quantiles"))
    finally:
        fit.close()


# ---- one larger shape ------------------------------------------------------------------------------------------------------------------------------------
def test_larger_shape_and_device_memory(hip_lib):
    rows, S, T = 200000, 8, 5
    args = rc.PREDICT_CASES["cap-exact"][0]()
    assert args.n_trees == T and args.iter - args.warmup == S
    chain = Chain(hip_lib, args, steps=(S,), rows=rows)
    try:
        assert len(chain.x) == rows
        probs, cols = (0.025, 0.5, 0.975), (_used_column(chain, S),)
        assert chain.counts(S, cols).sum() > 0
        got, *_ = _case(chain, (S,), rows, cols, "200000 rows", probs=probs, M=1, E=1, offset=True, arm0=("dense0",), G=2, scratch_bytes=1 << 20)
        nodes = struct.unpack_from("<Q", chain.live.export_bart_state(), 28)[0]
        info = got["info"]
        assert info["rows_per_chunk"] * 8 * S <= 1 << 20 and info["rows_per_chunk"] == 16384 and info["chunks"] == -(-rows // 16384)
        # link 0: of the linear parts only the dense one, whose arm-0 side was given, is uploaded and evaluated
        want = cc.device_bytes_formula(args.x_bart.shape[1], rows, nodes, S, T, info["rows_per_chunk"], D=1, M=1, dense0=True, G=2, Q=len(probs))
        print(f"device memory of the call: {info['device_bytes']} bytes, formula {want}; two draws matrices would add {2 * 8 * rows * S - 8 * info['rows_per_chunk'] * S}")
        assert info["device_bytes"] == want
    finally:
        chain.close()
