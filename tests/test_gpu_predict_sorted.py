"""s4b_predict_sorted on the device (stan4bart_amd/csrc/readout_sorted.inc: k_predict_values / k_contrast_values unchanged on a view of a block of
draws, k_sorted_hist, k_sorted_scan, k_sorted_count, k_sorted_finish, k_level_rows and k_row_quantiles unchanged over the statistics matrix) against
the numpy model of tests/sorted_cases.py.

A. The selection and count kernels ALONE through s4b_test_sorted_select on planted matrices: order statistics are compared as BITS, counts exactly.
B. The pooled call on small chains: the reference matrix is the device's own x(i, k), which predict_groups with every row its own level and statistic
   "sum" returns bit for bit.  The cut rows, n_above and n_below are asserted EQUAL to the model; a sorted row with g = 0 is the order statistic bit
   for bit, otherwise it lies within [y(lo), y(hi)] and within 4 units in the last place of max(|y(lo)|, |y(hi)|) of numpy's xl + g (xh - xl): each
   form rounds a product of magnitude <= 2 max and a sum of magnitude <= max, so each is within 1.5 such units of the exact value and two forms are
   within 3 (a contracted multiply-add rounds once instead of twice).  Blocks of 8 draws against one block give the same bits for every output: that
   is what proves the view of a block of draws.

The chain is tests/describe_cases.py's small_chain with 300 new rows: Gaussian, n = 100, 5 trees, 13 live draws, stored samplers of 1, 2, 5 and 13.
The issue's large shape, 262 401 rows, does not reach the tile stride of the value kernels (PS_GRID_MAX x PS_BLOCK is 2^20 rows, tests/stride_cases.py);
it is kept as stated and 2^20 + 65 rows are run beside it."""
import numpy as np
import pytest

import describe_cases as dc
import quantile_cases as qc
import readout_cases as rc
import sorted_cases as so
import summary_cases as sc

pytestmark = pytest.mark.gpu
PROBS = (0.025, 0.5, 0.975, 0.0, 1.0, 1.0 / 3.0)
ROW_PROBS = (0.1, 0.25, 0.5, 0.75, 0.9, 0.0, 1.0, 1.0 / 3.0)
COUNTS = ("n_above", "n_below")


@pytest.fixture(scope="module")
def chain(hip_lib):
    c = dc.Chain(hip_lib, "s4b_", rc._friedman(n=100, T=5, warmup=4, iter=4 + 13, ranef=False), rows=300, steps=(1, 1, 3, 8))
    yield c
    c.close()


# ================================================================ A. the kernels alone ========================================================================
def _select(smp, x, ranks=(), cuts=(), block=8, what=""):
    """The test entry on x [n x S] against the model: order statistics as bits, counts exactly; the launches as documented."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, S = x.shape
    got = smp.test_sorted_select(x, block, ranks=ranks, cut_rank=cuts)
    ref_r, ref_c = so.model(x, (), ranks), so.model(x, (), cuts)
    if len(ranks):
        bad = np.argwhere(got["order_stats"].view(np.uint64) != ref_r["cut"].view(np.uint64))
        assert len(bad) == 0, f"{what}: order_stats differs at {bad[:5].tolist()}: device {got['order_stats'][tuple(bad[0])]!r}, model {ref_r['cut'][tuple(bad[0])]!r}"
    for k in COUNTS:
        if len(cuts):
            bad = np.argwhere(got[k] != ref_c[k])
            assert got[k].dtype == np.int32 and len(bad) == 0, f"{what}: {k} differs at {bad[:5].tolist()}"
    info = got["info"]
    Db = min(block, S)
    distinct = len(set(int(r) for r in ranks) | set(int(c) for c in cuts))
    assert (info["draws_per_block"], info["blocks"], info["draws"], info["targets"], info["passes"]) == (Db, -(-S // Db), S, distinct, 8), info
    assert info["launches"] == info["blocks"] * (16 + (1 if len(cuts) else 0)) + (1 if len(ranks) else 0), info
    assert info["draws_per_workgroup"] == (8 if distinct <= 8 else 4 if distinct <= 16 else 2)
    return got


def _ranks(n):
    return sorted({0, n - 1, n // 2, max(0, n // 2 - 1), (9 * n) // 10, n // 10})


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 70001])
def test_select_row_counts(chain, n):
    g = np.random.default_rng(n)
    x = g.normal(size=(n, 5))
    x[:, 3] = 1.0 + g.random(n)          # one sign, one exponent: the first passes have one full bin, 70 001 in it (a count past 65 535)
    r = _ranks(n)
    _select(chain.stored[1], x, ranks=r, cuts=r[:8], block=8, what=f"{n} rows")


@pytest.mark.parametrize("S", [1, 5, 8, 13, 21])
def test_select_draw_counts_and_blocks(chain, S):
    n = 257
    x = np.random.default_rng(S).normal(size=(n, S))
    r = _ranks(n)
    a = _select(chain.stored[1], x, ranks=r, cuts=r[:3], block=8, what=f"{S} draws in blocks of 8")
    b = _select(chain.stored[1], x, ranks=r, cuts=r[:3], block=max(S, 8) + 3, what=f"{S} draws in one block")
    assert a["info"]["blocks"] == -(-S // 8) and b["info"]["blocks"] == 1
    assert so.same_bits(a["order_stats"], b["order_stats"]) and all(np.array_equal(a[k], b[k]) for k in COUNTS)


def test_select_all_equal_and_nearly(chain):
    n = 70001
    x = np.full((n, 3), 0.1)
    x[:, 1] = -2.5
    got = _select(chain.stored[1], x, ranks=(0, n // 2, n - 1), cuts=(n // 2,), what="all values equal")          # every pass: one full bin
    assert not got["n_above"].any() and not got["n_below"].any()
    y = np.full((n, 3), 0.1)
    y[::64, 0], y[5::64, 1], y[63::64, 2] = 0.1000001, -7.0, np.nextafter(0.1, 1.0)          # one value per 64 rows differs: no wave agrees entirely
    k = len(y[::64])
    _select(chain.stored[1], y, ranks=(0, 1, n - k - 1, n - k, n - 1, k - 1, k), cuts=(n - k - 1, k), what="all equal but one value per 64 rows")


@pytest.mark.parametrize("n", [256, 70001])
def test_select_decided_in_the_last_digit(chain, n):
    v = 0.3
    x = np.empty((n, 2))
    x[: n // 2], x[n // 2:] = v, np.nextafter(v, 1.0)
    x[:, 1] = x[::-1, 0]
    assert so.key(np.array([v]))[0] >> np.uint64(8) == so.key(np.array([np.nextafter(v, 1.0)]))[0] >> np.uint64(8)
    got = _select(chain.stored[1], x, ranks=(n // 2 - 1, n // 2), cuts=(n // 2 - 1, n // 2), what="x and nextafter(x)")
    assert np.all(got["order_stats"][0] == v) and np.all(got["order_stats"][1] == np.nextafter(v, 1.0))


def test_select_zeros_of_both_signs(chain):
    for name, p in so.PLANTED.items():
        got = chain.stored[1].test_sorted_select(np.array(p["x"]), 8, ranks=p["ranks"], cut_rank=p["cut_rank"])
        assert so.same_bits(got["order_stats"], np.array(p["order_stats"])), name
        assert np.array_equal(got["n_above"], np.array(p["n_above"])) and np.array_equal(got["n_below"], np.array(p["n_below"])), name
    g = np.random.default_rng(5)
    n = 300
    x = g.choice(np.array([0.0, -0.0, 1.5, -1.5]), size=(n, 6), p=(0.4, 0.4, 0.1, 0.1))
    x[:, 0] = np.where(g.random(n) < 0.5, 0.0, -0.0)          # a column of zeros only: the cut is a zero, nothing is above or below
    r = list(range(0, n, 13)) + [n - 1]
    got = _select(chain.stored[1], x, ranks=r, cuts=(n // 2, 0, n - 1, n // 4), what="zeros of both signs")
    y = so.sorted_columns(x)
    minus = int(np.signbit(x[:, 0]).sum())
    assert np.all(np.signbit(y[:minus, 0])) and not np.any(np.signbit(y[minus:, 0])), "the model's order of the zeros"
    assert np.array_equal(np.signbit(got["order_stats"][:, 0]), np.array(r) < minus), "the sign of the returned zero follows the key order"
    zeros = chain.stored[1].test_sorted_select(x[:, :1], 8, cut_rank=(n // 2, 0, n - 1))          # against a zero cut neither zero is above or below
    assert not zeros["n_above"].any() and not zeros["n_below"].any()


def test_select_extreme_and_random_bit_patterns(chain):
    g = np.random.default_rng(9)
    n = 1000
    bits = g.integers(0, 1 << 64, size=(n, 8), dtype=np.uint64)
    x = bits.view(np.float64).copy()
    bad = ~np.isfinite(x)
    x[bad] = g.normal(size=int(bad.sum()))          # (the values of a call are finite)
    big = np.finfo(np.float64).max
    x[:40, 1] = np.repeat([big, -big, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 0.0, -0.0], 5)
    x[:, 2] = g.choice(np.array([big, -big, 5e-324, -5e-324, 1e-310, -1e-310]), size=n)
    r = sorted(set(g.integers(0, n, 22).tolist()) | {0, n - 1})
    _select(chain.stored[1], x, ranks=r, cuts=r[:8], what="every digit position in play")


def test_select_ties_of_one_decimal(chain):
    g = np.random.default_rng(21)
    n = 513
    x = np.round(g.normal(size=(n, 9)), 1) + 0.0
    y = so.sorted_columns(x)
    inside = [r for r in range(1, n - 1) if y[r - 1, 0] == y[r, 0] == y[r + 1, 0]][:10]
    assert len(inside) == 10, "no rank inside a run of ties"
    got = _select(chain.stored[1], x, ranks=inside + [0, n - 1], cuts=inside[:4], what="ranks inside runs of ties")
    assert (got["n_above"][0] + got["n_below"][0]).sum() <= 9 * n - 3 * 9, "every cut ties with at least three values of its column"


def test_select_rank_lists(chain):
    g = np.random.default_rng(33)
    n = 700
    x = g.normal(size=(n, 11))
    smp = chain.stored[1]
    _select(smp, x, ranks=(n - 1, 0), cuts=(n - 1, 0), what="the extremes")
    _select(smp, x, ranks=(5, 5, 5, 699, 5), cuts=(5, 5, 100, 100), what="duplicates")
    _select(smp, x, ranks=(10, 11, 12, 13, 350, 351), cuts=(351, 350), what="adjacent pairs")
    _select(smp, x, ranks=(650, 3, 99, 98, 400, 7), cuts=(300, 2, 299), what="unsorted")
    full = g.permutation(n)[:32]
    got = _select(smp, x, ranks=full[:24], cuts=full[24:], what="32 targets")
    assert got["info"]["targets"] == 32 and got["info"]["draws_per_workgroup"] == 2
    with pytest.raises(RuntimeError, match="more than 32 distinct ranks"):
        smp.test_sorted_select(x, 8, ranks=np.arange(32), cut_rank=(32,))


# ================================================================ B. the pooled call ===========================================================================
_X = {}


def _arms(chain, lens, rows, arms=1, link=0, M=0, offset=False, col=None, seed=0, x=None):
    """The keyword arguments of a pooled call over `rows` rows; every occurrence of a pooled sampler gets a coefficient table of its own."""
    x1 = np.asfortranarray(chain.x[:rows] if x is None else x)
    tables = [sc.linear_parts(rows, S, M, 0, seed=seed + 100 * j) for j, S in enumerate(lens)]
    off = None
    if offset:
        g = np.random.default_rng(seed)
        off = g.normal(-14.0, 3.0, rows) if link else float(chain.range[1] - chain.range[0]) * g.uniform(-1.0, 1.0, rows)
    kw = dict(x_test=x1, offset=off, link=link, peers=[chain.stored[S] for S in lens[1:]], n_arms=arms, **tables[0])
    if M:
        kw["peer_dense_coef"] = [t["dense_coef"] for t in tables[1:]]
    if arms == 2:
        kw["x_test0"] = np.asfortranarray(chain.arm0(col)[:rows]) if col is not None else None
    return kw


def _x(first, kw, key=None, piece=65536):
    """The device's own x [rows x S] of a call's arms, bit for bit: predict_groups with every row its own level, the sum, in pieces of rows."""
    if key is not None and key in _X:
        return _X[key]
    rows = kw["x_test"].shape[0]
    parts = []
    for r0 in range(0, rows, piece):
        sl = slice(r0, min(rows, r0 + piece))
        sub = {k: (np.asfortranarray(v[sl]) if k in ("x_test", "x_test0", "dense") and v is not None else v[sl] if k == "offset" and v is not None else v)
               for k, v in kw.items()}
        m = sl.stop - sl.start
        parts.append(first.predict_groups(level=np.arange(m), n_levels=m, statistic="sum", probs=(), outputs=("draws",), presorted=True, **sub)["draws"])
    x = np.concatenate(parts, axis=0)
    if key is not None:
        _X[key] = x
        x.setflags(write=False)
    return x


def _check(got, x, row_probs, cuts, what):
    """The statistics matrix and the counts of a call against the model of the device's own values."""
    n, S = x.shape
    ref = so.model(x, row_probs, cuts)
    Qr, J = len(row_probs), len(cuts)
    D = got["draws"]
    assert D.shape == (Qr + J, S), (what, D.shape)
    assert so.same_bits(D[Qr:], ref["cut"]), f"{what}: a cut row is not the order statistic bit for bit"
    for k in COUNTS:
        bad = np.argwhere(got[k] != ref[k])
        assert got[k].dtype == np.int32 and got[k].shape == (J, n) and len(bad) == 0, f"{what}: {k} differs at {bad[:5].tolist()}"
    worst = 0.0
    for j in range(Qr):
        if ref["g"][j] == 0.0:
            assert so.same_bits(D[j], ref["lo"][j]), f"{what}: sorted row {j} (g = 0) is not the order statistic bit for bit"
            continue
        lo, hi = ref["lo"][j], ref["hi"][j]
        assert np.all((D[j] >= lo) & (D[j] <= hi)), f"{what}: sorted row {j} leaves [y(lo), y(hi)]"
        ulp = np.spacing(np.maximum(np.abs(lo), np.abs(hi)))
        with np.errstate(invalid="ignore", divide="ignore"):
            d = np.where(D[j] == ref["sorted"][j], 0.0, np.abs(D[j] - ref["sorted"][j]) / ulp)
        worst = max(worst, float(d.max()))
    print(f"{what}: cut rows and counts equal; sorted rows at most {worst:.3g} units in the last place from numpy's (allowed: 4)")
    assert worst <= 4.0, f"{what}: {worst:.3g} units in the last place"
    return ref


def _same_bits(a, b, what, keys=("draws", "mean", "m2", "quantiles") + COUNTS):
    for k in keys:
        assert (a.get(k) is None) == (b.get(k) is None), (what, k)
        if a.get(k) is not None:
            assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint64 if a[k].dtype == np.float64 else a[k].dtype),
                                                               b[k].view(np.uint64 if b[k].dtype == np.float64 else b[k].dtype)), f"{what}: {k} differs"


def _expect_info(info, n, S, row_probs, cuts, scratch=0, Q=len(PROBS)):
    Db = so.draws_per_block(n, S, scratch)
    assert (info["draws_per_block"], info["blocks"], info["draws"], info["passes"]) == (Db, -(-S // Db), S, 8), info
    assert info["targets"] == len(so.targets(n, row_probs, cuts)), info
    assert info["launches"] == so.launches(S, Db, counts=len(cuts) > 0, summary=1 + (1 if Q else 0)), info          # (k_level_rows and k_row_quantiles: one piece)
    assert info["device_bytes"] > 8 * n * Db


@pytest.mark.parametrize("link", [0, 1])
@pytest.mark.parametrize("arms", [1, 2])
def test_pooled_call_against_the_model(chain, arms, link):
    rows, lens = 101, (13, 5)
    S, first = sum(lens), chain.stored[13]
    extra = dict(col=chain.used_column(13)) if arms == 2 else {}
    kw = _arms(chain, lens, rows, arms=arms, link=link, M=2, offset=True, **extra)
    x = _x(first, kw, ("pooled", arms, link))
    assert x.shape == (rows, S) and len(np.unique(x)) > rows
    cuts = so.group_ranks(rows, top=(0.1, 0.07), bottom=(0.1,)) + [50, 0, rows - 1]
    call = dict(row_probs=ROW_PROBS, cut_rank=cuts, probs=PROBS, **kw)
    res = {}
    for route in ("staged", "global"):
        res[route] = first.predict_sorted(route=route, **call)
        assert res[route]["info"]["route"] == (1 if route == "staged" else 2)
    got = res["staged"]
    assert got["draws_pooled"] == S
    _expect_info(got["info"], rows, S, ROW_PROBS, cuts)
    ref = _check(got, x, ROW_PROBS, cuts, f"{arms} arm(s), link {link}, 101 rows, pool (13, 5)")
    assert so.type7_rows(0.5, rows)[2] == 0.0 and so.same_bits(got["draws"][2], so.sorted_columns(x)[50]), "n = 101 at p = 0.5 is an order statistic"
    assert ref["g"][7] != 0.0 and not ref["g"][:7].any(), "at 101 rows only the prob 1 / 3 falls between two ranks"
    _same_bits(res["staged"], res["global"], "the two routes")
    _same_bits(got, first.predict_sorted(route="staged", **call), "two calls")
    live = dict(call, peers=[chain.stored[5]])
    _same_bits(got, chain.live.predict_sorted(**live), "live and stored samplers")
    # p = 0 and p = 1 are predict_spread's min and max draws
    spread = first.predict_spread(thresholds=(), probs=(), outputs=("draws",), **{k: v for k, v in kw.items()})["draws"]
    assert so.same_bits(got["draws"][5], spread[2]) and so.same_bits(got["draws"][6], spread[3]), "p = 0 and p = 1 against predict_spread's min and max"
    # blocks of 8 draws (8 + 8 + 2 of 18 pooled) against one block
    cut = first.predict_sorted(scratch_bytes=1, **call)
    assert cut["info"]["draws_per_block"] == 8 and cut["info"]["blocks"] == 3 and got["info"]["blocks"] == 1
    _expect_info(cut["info"], rows, S, ROW_PROBS, cuts, scratch=1)
    _same_bits(got, cut, "one block and three")


def test_blocks_of_the_live_sampler_and_every_output_alone(chain):
    rows, S = 300, 13
    kw = _arms(chain, (S,), rows, M=1, offset=True)
    x = _x(chain.stored[13], kw, "live13")
    cuts = so.group_ranks(rows, top=(0.1,), bottom=(0.1,))
    call = dict(row_probs=ROW_PROBS, cut_rank=cuts, probs=PROBS, **kw)
    one = chain.live.predict_sorted(**call)
    cut = chain.live.predict_sorted(scratch_bytes=8 * rows * 8, **call)          # 8 + 5 of 13 pooled
    assert one["info"]["blocks"] == 1 and (cut["info"]["draws_per_block"], cut["info"]["blocks"]) == (8, 2)
    _check(cut, x, ROW_PROBS, cuts, "13 live draws in blocks of 8 and 5")
    _same_bits(one, cut, "one block and two")
    for k in ("mean", "m2", "quantiles", "draws") + COUNTS:
        alone = chain.live.predict_sorted(outputs=(k,), scratch_bytes=8 * rows * 8, **call)
        assert [n for n in ("mean", "m2", "quantiles", "draws") + COUNTS if alone[n] is not None] == [k]
        _same_bits(alone, cut, f"{k} alone", keys=(k,))
    # the binding's groups: without ties at the boundary exactly m rows of every draw lie beyond the cut
    grp = chain.live.predict_sorted(top=(0.1,), bottom=(0.1,), **kw)
    assert list(grp["cut_rank"]) == cuts and list(grp["top_count"]) == [30] and list(grp["bottom_count"]) == [30]
    assert np.array_equal(grp["n_above"], one["n_above"]) and np.array_equal(grp["p_top"], one["n_above"][:1] / S) and np.array_equal(grp["p_bottom"], one["n_below"][1:] / S)
    assert grp["n_above"][0].sum() == 30 * S and grp["n_below"][1].sum() == 30 * S


def test_peers_in_two_orders(chain):
    rows = 130
    cuts = so.group_ranks(rows, top=(0.1,), bottom=(0.2,))
    res, xs = {}, {}
    for lens in ((13, 5), (5, 13)):
        first = chain.stored[lens[0]]
        kw = _arms(chain, lens, rows)
        xs[lens] = _x(first, kw)
        res[lens] = first.predict_sorted(row_probs=ROW_PROBS, cut_rank=cuts, probs=PROBS, **kw)
        _check(res[lens], xs[lens], ROW_PROBS, cuts, f"peers {lens}")
    assert so.same_bits(xs[13, 5][:, :13], xs[5, 13][:, 5:]) and so.same_bits(xs[13, 5][:, 13:], xs[5, 13][:, :5])
    a, b = res[13, 5], res[5, 13]
    assert all(np.array_equal(a[k], b[k]) for k in COUNTS), "the counts depend on the order of the peers"
    assert so.same_bits(np.c_[a["draws"][:, 13:], a["draws"][:, :13]], b["draws"]), "the columns of the statistics matrix are permuted with the peers"
    assert so.same_bits(a["quantiles"], b["quantiles"])


def test_contrast_on_an_unused_predictor_is_all_zero(chain):
    rows = 200
    S, unused = next((S, u) for S in (13, 5, 2, 1) for u in [[j for j in range(chain.P) if chain.hit(S, [j]).sum() == 0]] if u)          # the most draws whose trees leave a predictor out
    kw = _arms(chain, (S,), rows, arms=2, col=unused[0])
    got = chain.stored[S].predict_sorted(row_probs=ROW_PROBS, cut_rank=(0, 100, 199), probs=PROBS, **kw)
    assert got["info"]["route"] == 0 and so.same_bits(got["draws"], np.zeros((len(ROW_PROBS) + 3, S))), "every order statistic is +0.0"
    assert not got["n_above"].any() and not got["n_below"].any() and not got["mean"].any() and not got["m2"].any() and not got["quantiles"].any()


def test_one_row(chain):
    S = 13
    kw = _arms(chain, (S,), 1, M=1)
    x = _x(chain.stored[S], kw)
    got = chain.stored[S].predict_sorted(row_probs=(0.0, 0.3, 1.0), cut_rank=(0,), probs=PROBS, **kw)
    assert got["info"]["targets"] == 1
    for j in range(4):
        assert so.same_bits(got["draws"][j], x[0])
    assert not got["n_above"].any() and not got["n_below"].any()


@pytest.mark.parametrize("rows", [262401, (1 << 20) + 65])
def test_many_rows(chain, rows):
    """262 401 rows as the issue states them; 2^20 + 65 rows, where a workgroup of the value kernel takes a second tile (PS_GRID_MAX x PS_BLOCK rows and
    more).  Few trees (5), few draws; the reference is the device's own matrix taken in pieces of rows."""
    S = 13 if rows < (1 << 20) else 5
    g = np.random.default_rng(rows)
    xb = chain.args.x_bart
    x_new = np.asfortranarray(np.column_stack([xb[g.integers(0, len(xb), rows), j] + 1e-3 * g.normal(size=rows) for j in range(chain.P)]))
    first = chain.stored[S]
    kw = _arms(chain, (S,), rows, x=x_new)
    x = _x(first, kw)
    cuts = so.group_ranks(rows, top=(0.1,), bottom=(0.1,))
    got = first.predict_sorted(row_probs=(0.1, 0.5, 0.9), cut_rank=cuts, probs=(0.5,), **kw)
    Db = so.draws_per_block(rows, S)
    assert got["info"]["draws_per_block"] == Db and got["info"]["blocks"] == -(-S // Db)
    _check(got, x, (0.1, 0.5, 0.9), cuts, f"{rows} rows, {S} draws")
    if rows < (1 << 20):
        few = first.predict_sorted(row_probs=(0.1, 0.5, 0.9), cut_rank=cuts, probs=(0.5,), scratch_bytes=1, **kw)
        assert few["info"]["draws_per_block"] == 8 and few["info"]["blocks"] == 2
        _same_bits(got, few, "one block and two at 262 401 rows")


def test_summary_over_the_draws(chain):
    """mean, m2 and quantiles over the draws against the returned draws, with the model and the bound tests/test_gpu_predict_spread.py uses for its
    matrix (summary_cases.summarise, quantile_cases.type7 / bound; the matrix itself is taken as exact)."""
    rows, lens = 300, (13, 5, 2, 1)
    first = chain.stored[13]
    kw = _arms(chain, lens, rows, arms=2, col=chain.used_column(13), M=1)
    got = first.predict_sorted(row_probs=ROW_PROBS, cut_rank=(30, 269), probs=PROBS, **kw)
    D = got["draws"]
    assert D.shape == (len(ROW_PROBS) + 2, 21)
    zero = np.zeros_like(D)
    r, b = sc.summarise(D, zero)
    ratios = dict(mean=rc.bound_ratio(got["mean"], r["mean"], b["mean"]), m2=rc.bound_ratio(got["m2"], r["m2"], b["m2"]),
                  quantiles=rc.bound_ratio(got["quantiles"], qc.type7(D, PROBS).astype(np.float64), qc.bound(D, zero, len(PROBS))))
    print("predict_sorted, over the draws, max |device - model| / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert max(ratios.values()) <= rc.BOUND_FACTOR, ratios
    assert got["quantiles"].shape == (len(PROBS), len(ROW_PROBS) + 2)
    assert so.same_bits(got["quantiles"][3], D.min(axis=1)) and so.same_bits(got["quantiles"][4], D.max(axis=1))


def test_refusals_and_the_query_launch_nothing(chain):
    rows = 300
    x = np.asfortranarray(chain.x[:rows])
    live = chain.live

    def refused(match, **kw):
        before = live.get_counters()
        args = dict(x_test=x, row_probs=(0.5,), cut_rank=(3,), probs=(0.5,))
        args.update(kw)
        with pytest.raises(RuntimeError, match=match):
            live.predict_sorted(**args)
        assert not any(live.sorted_info.values()), live.sorted_info
        assert np.array_equal(live.get_counters(), before), "a refused call launched something"

    refused(r"predict_sorted: n_row_probs must lie in \[0, 12\], not 13", row_probs=np.linspace(0, 1, 13))
    refused(r"predict_sorted: n_cuts must lie in \[0, 8\], not 9", cut_rank=[1] * 9)
    refused(r"predict_sorted: row prob nan outside \[0, 1\]", row_probs=(np.nan,))
    refused(r"predict_sorted: cut_rank 300 outside \[0, 299\]", cut_rank=(300,))
    refused("predict_sorted: n_arms must be 1 .* or 2 .*, not 3", n_arms=3)
    refused("predict_sorted: n_arms = 1 takes no arm-0 pointer", x_test0=x)
    refused("predict_sorted: arms.rows.n_weights must be 0", weights=np.ones(rows))
    refused("negative scratch_bytes", scratch_bytes=-1)
    before = live.get_counters()
    plan = live.predict_sorted(x, row_probs=ROW_PROBS, cut_rank=(3, 7), probs=PROBS, outputs=(), scratch_bytes=8 * rows * 8)
    assert all(plan[k] is None for k in ("mean", "m2", "quantiles", "draws") + COUNTS) and plan["draws_pooled"] == 13
    info = plan["info"]
    assert info["launches"] == 0 and info["device_bytes"] == 0 and (info["draws_per_block"], info["blocks"], info["draws"], info["passes"]) == (8, 2, 13, 8), info
    assert info["targets"] == len(so.targets(rows, ROW_PROBS, (3, 7))) and info["route"] in (1, 2)
    assert np.array_equal(live.get_counters(), before), "the query launched something"
    done = live.predict_sorted(x, row_probs=ROW_PROBS, cut_rank=(3, 7), probs=PROBS, scratch_bytes=8 * rows * 8)
    assert {k: v for k, v in done["info"].items() if k not in ("launches", "device_bytes")} == {k: v for k, v in info.items() if k not in ("launches", "device_bytes")}
    assert live.get_counters()[2] == before[2] + done["info"]["launches"]
    assert live.sorted_draws() == 13 and chain.stored[5].sorted_draws() == 5


def test_predict_sorted_end_to_end(hip_lib):
    """Stan4bartFit.predict_sorted against the model of the device's own values (fit.predict_groups with every row its own level, the sum, of the
    same seed): one arm and a treatment, two chains pooled."""
    from stan4bart_amd import GroupTerm, generate_friedman_data
    from stan4bart_amd.abi import Sampler
    from stan4bart_amd.generics import stan4bart
    d = generate_friedman_data(120, ranef=True, causal=True, p=10)
    x, z = d["x"], np.asarray(d["z"], dtype=np.float64)
    xb, X = np.column_stack([x[:, [j for j in range(10) if j != 3]], z]), np.column_stack([x[:, 3], z])
    groups = [GroupTerm(d["g1"], None, "g.1"), GroupTerm(d["g2"], None, "g.2")]
    fit = stan4bart(d["y"], xb, X=X, groups=groups, chains=2, seed=99, iter=11, warmup=6, bart_args={"n.trees": 9, "keepTrees": True},
                    make_sampler=lambda a, st: Sampler(hip_lib, "s4b_", a, st))
    try:
        m = 90
        g = np.random.default_rng(11)
        xb1, X1, off = rc.new_rows(xb, m, seed=4), X[:m] + g.normal(size=(m, 2)), g.normal(size=m)
        new = [GroupTerm(np.asarray(d["g1"])[:m], None, "g.1"), GroupTerm(np.asarray(d["g2"])[:m], None, "g.2")]
        for name, arms in (("one arm", {}), ("treatment", dict(treatment=("x_bart", 9)))):
            common = dict(X=X1, groups=new, offset=off, seed=7, **arms)
            vals = fit.predict_groups(np.arange(m), xb1, statistic="sum", return_draws=True, probs=(), **common)["average"]
            S = vals.shape[1]
            assert S == 10
            got = fit.predict_sorted(xb1, top=(0.1, 0.07), bottom=(0.2,), return_draws=True, **common)
            assert got["draws"] == S and list(got["top_count"]) == [9, 7] and list(got["bottom_count"]) == [18] and list(got["cut_rank"]) == [80, 82, 18], name
            ref = so.model(vals, got["row_probs"], got["cut_rank"])
            assert so.same_bits(got["cut"]["draws"], ref["cut"]) and np.array_equal(got["n_above"], ref["n_above"]) and np.array_equal(got["n_below"], ref["n_below"]), name
            assert np.array_equal(got["p_top"], ref["n_above"][:2].astype(np.int64) / S) and np.array_equal(got["p_bottom"], ref["n_below"][2:].astype(np.int64) / S), name
            np.testing.assert_allclose(got["sorted"]["draws"], ref["sorted"], rtol=1e-13, atol=1e-14)
            np.testing.assert_allclose(got["sorted"]["mean"], ref["sorted"].mean(axis=1), rtol=1e-12)
            np.testing.assert_allclose(got["sorted"]["sd"], ref["sorted"].std(axis=1, ddof=1), rtol=1e-10)
            np.testing.assert_allclose(got["cut"]["quantiles"], np.quantile(ref["cut"], (0.025, 0.5, 0.975), axis=1), rtol=1e-12)
            brief = fit.predict_sorted(xb1, top=(0.1, 0.07), bottom=(0.2,), **common)
            assert "draws" not in brief["sorted"] and np.array_equal(brief["p_top"], got["p_top"]) and np.array_equal(brief["sorted"]["mean"], got["sorted"]["mean"]), name
    finally:
        fit.close()
