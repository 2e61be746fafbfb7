"""s4b_predict_describe on the device (stan4bart_amd/csrc/readout_describe.inc: k_predict_values / k_contrast_values unchanged, k_row_describe) against
the numpy model of tests/describe_cases.py, EXACTLY: the reference matrix is the device's own x(i, k), which predict_groups with every row its own
level and statistic "sum" returns bit for bit, and every output is a function of the sorted row that numpy forms with the same operations.  hdi,
hdi_start, n_above, n_below, median and mad are asserted equal; quantiles equal to predict_quantiles' / predict_contrast's bits.  No tolerance anywhere.

The smallest shapes at which the kernel can go wrong: 1 .. 16 384 pooled draws (Sp = S and just above it, R = 4 096 .. 1 rows per sort workgroup, the
largest LDS request) at 70 rows (the last sort workgroup partial wherever R > 1); three chunks whose last is no multiple of R; both routes, live and
stored samplers, two calls, permuted peers; series planted exactly with their values written out by hand; link 1 with the arms swapped; the refusals
and the query before any launch; the device bytes; the Python interface.

The chains of tests/test_gpu_predict_groups.py: Gaussian, n = 100, 5 trees, stored samplers of 1, 7, 8, 9, 255, 257 and 2 048 draws; binary, n = 400,
11 trees, 1, 2, 5 and 13 draws."""
import math
import struct

import numpy as np
import pytest

import contrast_cases as cc
import describe_cases as dc
import quantile_cases as qc
import readout_cases as rc
import summary_cases as sc

pytestmark = pytest.mark.gpu
PROBS = (0.025, 0.5, 0.975, 0.0, 1.0, 1.0 / 3.0)
EXACT = ("median", "mad", "hdi", "hdi_start", "n_above", "n_below")
ALL = EXACT + ("quantiles",)


@pytest.fixture(scope="module")
def gauss(hip_lib):
    c = dc.gauss_chain(hip_lib)
    yield c
    c.close()


@pytest.fixture(scope="module")
def binary(hip_lib):
    c = dc.binary_chain(hip_lib)
    yield c
    c.close()


_X = {}


def _arms(chain, lens, rows, arms=1, link=0, M=0, offset=False, col=None, dense0=False, swap=False, seed=0):
    """The keyword arguments of a pooled call over the first `rows` rows.  Every OCCURRENCE of a pooled sampler gets a coefficient table of its own.  Two
    arms: column `col` of the BART rows differs (None: no BART column), `dense0`: arm 0 has a dense part of its own; `swap` exchanges the arms."""
    x1 = np.asfortranarray(chain.x[:rows])
    tables = [sc.linear_parts(rows, S, M, 0, seed=seed + 100 * j) for j, S in enumerate(lens)]
    off = float(chain.range[1] - chain.range[0]) * np.random.default_rng(seed).uniform(-1.0, 1.0, rows) if offset else None
    kw = dict(x_test=x1, offset=off, link=link, peers=[chain.stored[S] for S in lens[1:]], n_arms=arms, **tables[0])
    if M:
        kw["peer_dense_coef"] = [t["dense_coef"] for t in tables[1:]]
    if arms == 2:
        x0 = np.asfortranarray(chain.arm0(col)[:rows]) if col is not None else None
        d0 = sc.linear_parts(rows, 1, M, 0, seed=seed + 50)["dense"] if dense0 else None
        kw.update(x_test0=x0, dense0=d0)
        if swap:
            if x0 is not None:
                kw["x_test"], kw["x_test0"] = x0, x1
            if dense0:
                kw["dense"], kw["dense0"] = kw["dense0"], kw["dense"]
    return kw


def _x(first, kw, key=None):
    """The device's own x [rows x S] of a call's arms, bit for bit: predict_groups with every row its own level, the sum (computed once per key)."""
    if key is None or key not in _X:
        rows = kw["x_test"].shape[0]
        g = first.predict_groups(level=np.arange(rows), n_levels=rows, statistic="sum", probs=(), outputs=("draws",), presorted=True, **kw)
        if key is None:
            return g["draws"]
        _X[key] = g["draws"]
        _X[key].setflags(write=False)
    return _X[key]


def _counts(S):
    return sorted({1, math.ceil(0.5 * S), dc.hdi_draws(0.95, S), S})


def _check(got, x, counts, thresholds, what):
    ref = dc.model(x, counts, thresholds)
    for k in EXACT:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (what, k, got[k].shape, ref[k].shape)
        bad = np.argwhere(got[k] != ref[k])
        print(f"{what}: {k}: {len(bad)} of {got[k].size} entries differ from the model")
        assert len(bad) == 0, f"{what}: {k} differs at {bad[:5].tolist()}: device {got[k][tuple(bad[0])]!r}, model {ref[k][tuple(bad[0])]!r}"
    return ref


def _same_bits(a, b, what, keys=ALL):
    for k in keys:
        assert (a.get(k) is None) == (b.get(k) is None), (what, k)
        if a.get(k) is not None:
            assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k} differs"


# ---- the whole family against the model ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arms", [1, 2])
def test_whole_family_against_the_model(gauss, arms):
    rows, lens = 300, (9, 7)
    S, first = sum(lens), gauss.stored[9]
    kw = _arms(gauss, lens, rows, arms=arms, M=2, offset=True, **(dict(col=gauss.used_column(9), dense0=True) if arms == 2 else {}))
    x = _x(first, kw, ("family", arms))
    assert x.shape == (rows, S)
    counts = [1, math.ceil(0.5 * S), math.ceil(0.95 * S), S]
    thresholds = (dc.midpoint(x), float(x[17, 3]), float(np.median(x)), -np.inf, np.inf)
    got = first.predict_describe(hdi_count=counts, thresholds=thresholds, probs=PROBS, **kw)
    assert got["draws"] == S and got["info"]["draws"] == S and got["info"]["launches"] == 2 and got["info"]["chunks"] == 1, got["info"]
    assert (got["info"]["rows_per_sort"], got["info"]["padded_draws"]) == (256, 16)
    ref = _check(got, x, counts, thresholds, f"{arms} arm(s), 300 rows, pool (9, 7)")
    assert ref["n_above"][1, 17] + ref["n_below"][1, 17] < S, "the threshold on a value ties with no draw: the case does not test what it says"
    assert np.array_equal(got["n_above"][3], np.full(rows, S)) and not got["n_below"][3].any() and not got["n_above"][4].any()
    pooled = {k: v for k, v in kw.items() if k != "n_arms"}
    q = first.predict_quantiles(probs=PROBS, **pooled) if arms == 1 else first.predict_contrast(probs=PROBS, **pooled)
    assert np.array_equal(got["quantiles"], q["quantiles"]), "the quantiles are not the quantile call's bits"
    assert np.array_equal(got["median"], got["quantiles"][PROBS.index(0.5)]), "the median is not the quantile at 0.5"
    # every output alone returns what it returns in company; the MAD does not disturb what is read before it
    for k in ALL:
        alone = first.predict_describe(hdi_count=counts, thresholds=thresholds, probs=PROBS, outputs=(k,), **kw)
        assert [n for n in ALL if alone[n] is not None] == [k] and np.array_equal(alone[k], got[k]), f"{k} alone differs"


# ---- draw counts ---------------------------------------------------------------------------------------------------------------------------------------------
POOLS = {1: (1,), 2: (1, 1), 7: (7,), 8: (8,), 9: (9,), 255: (255,), 257: (257,), 2048: (2048,), 4097: (2048, 2048, 1), 16384: (2048,) * 8}


@pytest.mark.parametrize("S", sorted(POOLS))
def test_draw_counts(gauss, S):
    rows, lens = 70, POOLS[S]
    first = gauss.stored[lens[0]]
    kw = _arms(gauss, lens, rows)
    x = _x(first, kw)
    assert x.shape == (rows, S)
    counts = _counts(S)
    thresholds = (float(np.median(x)), float(x[69, S // 2]))
    got = first.predict_describe(hdi_count=counts, thresholds=thresholds, probs=(0.5, 0.9), **kw)
    info = got["info"]
    Sp = 1 << (S - 1).bit_length()
    R = max(1, 4096 // Sp)
    assert (info["padded_draws"], info["rows_per_sort"], info["sort_lds_bytes"]) == (Sp, R, 8 * max(Sp, 4096) + 8 * R), info
    _check(got, x, counts, thresholds, f"{S} pooled draws")
    assert np.array_equal(got["quantiles"], first.predict_quantiles(probs=(0.5, 0.9), **{k: v for k, v in kw.items() if k != "n_arms"})["quantiles"])
    if S == 1:
        assert np.array_equal(got["hdi"][0, 0], x[:, 0]) and np.array_equal(got["hdi"][0, 1], x[:, 0]) and np.array_equal(got["median"], x[:, 0])
        assert not got["mad"].any() and not got["hdi_start"].any()
    if S == 16384:
        assert info["sort_lds_bytes"] == 128 * 1024 + 8          # the largest request


# ---- chunking ------------------------------------------------------------------------------------------------------------------------------------------------
def test_chunking(gauss):
    rows, S = 1100, 9
    first = gauss.stored[S]
    kw = _arms(gauss, (S,), rows, M=2, offset=True)
    x = _x(first, kw, "chunking")
    counts, thresholds = _counts(S), (float(np.median(x)), 0.0)
    one = first.predict_describe(hdi_count=counts, thresholds=thresholds, probs=PROBS, **kw)
    cut = first.predict_describe(hdi_count=counts, thresholds=thresholds, probs=PROBS, scratch_bytes=384 * 8 * S, **kw)
    assert one["info"]["chunks"] == 1 and one["info"]["launches"] == 2 and one["info"]["rows_per_chunk"] == rows, one["info"]
    info = cut["info"]
    assert info["rows_per_chunk"] == 384 and info["chunks"] == 3 and info["launches"] == 6 and info["rows_per_sort"] == 256, info
    assert (rows - 2 * 384) % info["rows_per_sort"] != 0          # the last chunk ends on a partial sort workgroup
    _check(cut, x, counts, thresholds, "1100 rows in three chunks")
    _same_bits(one, cut, "one chunk and three")
    small = first.predict_describe(hdi_count=counts, thresholds=thresholds, probs=PROBS, scratch_bytes=1, **kw)
    assert small["info"]["rows_per_chunk"] == 64 and small["info"]["chunks"] == 18
    _same_bits(one, small, "one chunk and eighteen")


# ---- routes and samplers -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arms", [1, 2])
def test_routes_live_and_stored_two_calls(binary, arms):
    rows, S = 300, 13
    first = binary.stored[S]
    kw = _arms(binary, (S,), rows, arms=arms, M=1, **(dict(col=binary.used_column(S)) if arms == 2 else {}))
    x = _x(first, kw)
    call = dict(hdi_count=_counts(S), thresholds=(float(np.median(x)), dc.midpoint(x)), probs=PROBS, **kw)
    res = {}
    for route in ("staged", "global"):
        res[route] = first.predict_describe(route=route, **call)
        assert res[route]["info"]["route"] == (1 if route == "staged" else 2)
    _check(res["staged"], x, call["hdi_count"], call["thresholds"], f"{arms} arm(s), staged")
    _same_bits(res["staged"], res["global"], "the two routes")
    _same_bits(res["global"], first.predict_describe(route="global", **call), "two calls")
    _same_bits(res["staged"], binary.live.predict_describe(**call), "live and stored samplers")


def test_peers_permuted(gauss):
    rows = 130
    counts, res = _counts(16), {}
    x = _x(gauss.stored[7], _arms(gauss, (7, 9), rows))
    thresholds = (float(np.median(x)), dc.midpoint(x))
    for lens in ((7, 9), (9, 7)):
        res[lens] = gauss.stored[lens[0]].predict_describe(hdi_count=counts, thresholds=thresholds, probs=PROBS, **_arms(gauss, lens, rows))
    _check(res[7, 9], x, counts, thresholds, "peers 7, 9")
    _same_bits(res[7, 9], res[9, 7], "permuted peers")          # hdi_start included: it is an index into the SORTED row


# ---- exactly planted series ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", sorted(dc.PLANTED))
def test_planted_rows(gauss, S):
    """The one-hot dense columns of test_planted_series_ties_and_infinite_thresholds: per planted row a column that takes the BART part out exactly
    (bart + 1 x (-bart) = 0) and a column that adds the series.  1 100 rows at R = 512 rows per sort workgroup: the last workgroup holds 76 rows, one of
    them planted."""
    rows, group = 1100, dc.PLANTED[S]
    at = dict(zip(group["rows"], (3, 600, 1090)))
    bart = gauss.bart(S)[:rows]
    dense, coef = np.zeros((rows, 2 * len(at))), np.zeros((S, 2 * len(at)))
    for j, (name, i) in enumerate(at.items()):
        dense[i, 2 * j] = dense[i, 2 * j + 1] = 1.0
        coef[:, 2 * j], coef[:, 2 * j + 1] = -bart[i], group["rows"][name][0]
    smp = gauss.stored[S]
    kw = dict(x_test=np.asfortranarray(gauss.x[:rows]), dense=dense, dense_coef=coef)
    x = _x(smp, kw)
    got = smp.predict_describe(hdi_count=group["counts"], thresholds=group["thresholds"], probs=(0.5,), **kw)
    assert got["info"]["rows_per_sort"] == 512 and 1090 >= 2 * 512
    for name, i in at.items():
        assert np.array_equal(x[i], group["rows"][name][0]), f"{name}: the planted series did not arrive bit for bit"
        dc.assert_planted(got, S, name, i)
        ties = [int(np.sum(x[i] == t)) for t in group["thresholds"]]
        assert [int(a + b) for a, b in zip(got["n_above"][:, i], got["n_below"][:, i])] == [S - t for t in ties], name
    _check(got, x, group["counts"], group["thresholds"], f"planted rows, {S} draws")
    assert 1 in group["counts"] and S in group["counts"]


# ---- link 1 and swapped arms ---------------------------------------------------------------------------------------------------------------------------------
def test_link_1_and_swapped_arms(binary):
    """Swapping the arms negates every d bit for bit, so the sorted row is reversed and negated.  At ODD S the median is one order statistic: it is negated.
    Where the smallest width is attained by ONE window the window is mirrored: the ends are negated and exchanged, the start becomes S - m - start.
    n_above(t) becomes n_below(-t).  The deviations from the median are the same numbers: the MAD is unchanged."""
    rows, lens = 300, (5, 13, 5)
    S, first = sum(lens), binary.stored[5]
    assert S % 2 == 1
    one = _arms(binary, lens, rows, link=1, M=2, offset=True)
    x1 = _x(first, one)
    got1 = first.predict_describe(hdi_count=_counts(S), thresholds=(0.5, dc.midpoint(x1)), probs=PROBS, **one)
    _check(got1, x1, _counts(S), (0.5, dc.midpoint(x1)), "link 1, one arm")
    assert np.all((x1 > 0.0) & (x1 < 1.0))
    col = binary.used_column(13)
    for name, values in (("a BART column", dict(col=col)), ("a dense column only", dict(dense0=True))):
        kw = _arms(binary, lens, rows, arms=2, link=1, M=2, **values)
        x = _x(first, kw)
        counts = _counts(S)
        t = (dc.midpoint(x), 0.0, 0.01)
        a = first.predict_describe(hdi_count=counts, thresholds=t, probs=PROBS, **kw)
        _check(a, x, counts, t, f"link 1, two arms, {name}")
        swapped = _arms(binary, lens, rows, arms=2, link=1, M=2, swap=True, **values)
        assert np.array_equal(_x(first, swapped), -x), f"{name}: swapped arms do not negate bit for bit"
        b = first.predict_describe(hdi_count=counts, thresholds=[-v for v in t], probs=PROBS, **swapped)
        assert np.any(x != 0.0)
        assert np.array_equal(b["median"], -a["median"]) and np.array_equal(b["mad"], a["mad"]), name
        assert np.array_equal(b["n_above"], a["n_below"]) and np.array_equal(b["n_below"], a["n_above"]), name
        for c, m in enumerate(counts):
            ok = dc.unique_minimum(x, m)
            assert ok.sum() >= (rows if m == S else 1 if m > 1 else 0), (name, m, int(ok.sum()))          # (m = 1: every window has width 0, none is unique)
            assert np.array_equal(b["hdi"][c, 0, ok], -a["hdi"][c, 1, ok]) and np.array_equal(b["hdi"][c, 1, ok], -a["hdi"][c, 0, ok]), (name, m)
            assert np.array_equal(b["hdi_start"][c, ok], S - m - a["hdi_start"][c, ok]), (name, m)


# ---- refusals and the query ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(gauss):
    rows, S = 300, 9
    x = np.asfortranarray(gauss.x[:rows])
    live, smp = gauss.live, gauss.stored[S]
    own = live.describe_draws()
    assert own == 2048 and smp.describe_draws() == S

    def refused(match, **kw):
        before = live.get_counters()
        for s, n in ((live, own), (smp, S)):
            args = dict(x_test=x, hdi_count=(1,), thresholds=(0.0,), probs=(0.5,))
            args.update({k: (v(n) if callable(v) else v) for k, v in kw.items()})
            with pytest.raises(RuntimeError, match=match(n) if callable(match) else match):
                s.predict_describe(**args)
            assert not any(s.describe_info.values()), s.describe_info
        assert np.array_equal(live.get_counters(), before), "a refused call launched something"

    refused(r"predict_describe: n_hdi must lie in \[0, 8\], not 9", hdi_count=[1] * 9)
    refused(r"predict_describe: n_thresholds must lie in \[0, 32\], not 33", thresholds=np.arange(33.0))
    refused("between 0 and 16 probs per call, not 17", probs=np.linspace(0, 1, 17))
    refused(lambda n: rf"predict_describe: hdi_count 0 outside \[1, {n}\]", hdi_count=(1, 0))
    refused(lambda n: rf"predict_describe: hdi_count {n + 1} outside \[1, {n}\]", hdi_count=lambda n: (n + 1,))
    refused("predict_describe: threshold 1 is a NaN", thresholds=(0.0, np.nan))
    refused("predict_describe: n_arms must be 1 .* or 2 .*, not 0", n_arms=0)
    refused("predict_describe: n_arms must be 1 .* or 2 .*, not 3", n_arms=3)
    refused("predict_describe: n_arms = 1 takes no arm-0 pointer", x_test0=x)
    refused("predict_describe: n_arms = 1 takes no arm-0 pointer", offset=np.zeros(rows), offset0=np.zeros(rows))
    refused("predict_describe: arms.rows.n_weights must be 0", weights=np.ones(rows))
    refused("offset0 given, but arm 1 has no offset", n_arms=2, offset0=np.zeros(rows))
    three = x.copy()
    three[:, :3] += 10.0
    refused("the arms differ in 3 BART columns", n_arms=2, x_test0=three)
    refused("negative scratch_bytes", scratch_bytes=-1)
    refused("pooled draws, at most 16384", peers=[gauss.stored[2048]] * 8)
    before = live.get_counters()
    ok = smp.predict_describe(x_test=x, hdi_count=(S,), thresholds=(0.0,), probs=(0.5,))
    assert ok["info"]["launches"] == 2
    live.predict_describe(x_test=x, hdi_count=(1,), outputs=("hdi",))
    assert live.get_counters()[2] == before[2] + 2


def test_query_form_returns_the_plan_without_a_launch(gauss):
    rows, lens = 1100, (9, 7)
    first = gauss.stored[9]
    kw = _arms(gauss, lens, rows, M=2, offset=True)
    before = gauss.live.get_counters()
    plan = first.predict_describe(hdi_count=(3,), thresholds=(0.0,), probs=PROBS, outputs=(), scratch_bytes=384 * 8 * 16, **kw)
    assert all(plan[k] is None for k in ALL) and plan["draws"] == 16
    info = plan["info"]
    assert info["launches"] == 0 and info["device_bytes"] == 0, info
    assert (info["rows_per_chunk"], info["chunks"], info["draws"], info["rows_per_sort"], info["padded_draws"]) == (384, 3, 16, 256, 16), info
    assert info["sort_lds_bytes"] == 8 * 4096 + 8 * 256 and info["route"] in (1, 2)
    live = gauss.live.predict_describe(kw["x_test"], hdi_count=(2048,), thresholds=(0.0,), outputs=())          # the live sampler counts its launches
    assert live["info"]["launches"] == 0 and live["info"]["padded_draws"] == 2048 and live["draws"] == 2048, live["info"]
    assert np.array_equal(gauss.live.get_counters(), before), "the query launched something"
    done = first.predict_describe(hdi_count=(3,), thresholds=(0.0,), probs=PROBS, scratch_bytes=384 * 8 * 16, **kw)
    assert {k: v for k, v in done["info"].items() if k not in ("launches", "device_bytes")} == {k: v for k, v in info.items() if k not in ("launches", "device_bytes")}
    assert first.describe_draws() == 9          # without an input: the kept draws of the sampler alone


# ---- device bytes --------------------------------------------------------------------------------------------------------------------------------------------
def test_device_bytes(gauss):
    rows, S, T = 1100, 9, gauss.T
    first = gauss.stored[S]
    nodes = struct.unpack_from("<Q", first.export_bart_state(), 28)[0]
    counts, thresholds = (1, 5, 9), (0.0, 1.0)
    kw = _arms(gauss, (S,), rows, M=2, offset=True)
    got = first.predict_describe(hdi_count=counts, thresholds=thresholds, probs=PROBS, scratch_bytes=128 * 8 * S, **kw)
    C, Q = got["info"]["rows_per_chunk"], len(PROBS)
    assert C == 128
    value = qc.device_bytes_formula(gauss.P, rows, nodes, S, T, True, 2, 0, 0, C, 0) - 2 * 16          # (no quantiles per row, no probs there)
    want = dc.device_bytes_formula(value, rows, S, Q=Q, C=len(counts), T=len(thresholds), outputs=ALL)
    print(f"device memory of the call: {got['info']['device_bytes']} bytes, the sum of DESIGN.md 5.17: {want}; the draws matrix would take {8 * rows * S}")
    assert got["info"]["device_bytes"] == want
    few = first.predict_describe(hdi_count=counts, thresholds=thresholds, probs=PROBS, scratch_bytes=128 * 8 * S, outputs=("hdi", "n_above"), **kw)
    assert few["info"]["device_bytes"] == dc.device_bytes_formula(value, rows, S, Q=Q, C=len(counts), T=len(thresholds), outputs=("hdi", "n_above"))
    two = first.predict_describe(hdi_count=counts, thresholds=thresholds, probs=PROBS, scratch_bytes=128 * 8 * S,
                                 **_arms(gauss, (S,), rows, arms=2, col=gauss.used_column(S)))
    value = cc.device_bytes_formula(gauss.P, rows, nodes, S, T, 128, D=1, per_row=False)
    assert two["info"]["device_bytes"] == dc.device_bytes_formula(value, rows, S, Q=Q, C=len(counts), T=len(thresholds), outputs=ALL), two["info"]


# ---- the Python interface ------------------------------------------------------------------------------------------------------------------------------------
def test_describe_posterior_end_to_end(hip_lib):
    """Stan4bartFit.describe_posterior against the integer composition of the shares, formed here from the device's own values (fit.predict_groups with
    every row its own level, the sum, of the same seed): ci = 0.7 at 10 pooled draws is 7 draws, a ROPE, treatment=."""
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
            q = [float(v) for v in np.quantile(vals, (0.3, 0.5, 0.6, 0.8))]          # (values of the matrix or between them: some draws lie inside the ROPE, some outside)
            rope, thr, ci = (q[0], q[2]), (q[1], q[3]), (0.7, 0.95, 1.0)
            got = fit.describe_posterior(xb1, ci=ci, thresholds=thr, rope=rope, probs=(0.1, 0.5), mad_constant=1.4826, **common)
            assert got["draws"] == S and list(got["hdi_draws"]) == [7, 10, 10], name
            counts = [int(v) for v in got["hdi_draws"]]
            ref = dc.model(vals, counts, thr + (0.0,) + rope)
            assert np.array_equal(got["hdi"], ref["hdi"]) and np.array_equal(got["hdi_start"], ref["hdi_start"]) and np.array_equal(got["median"], ref["median"]), name
            assert np.array_equal(got["mad"], ref["mad"] * 1.4826) and np.array_equal(got["quantiles"][1], got["median"]), name
            na, nb = ref["n_above"].astype(np.int64), ref["n_below"].astype(np.int64)
            assert np.array_equal(got["p_above"], na[:2] / S) and np.array_equal(got["p_below"], nb[:2] / S), name
            assert np.array_equal(got["pd"], np.maximum(na[2], nb[2]) / S), name
            inside = ((vals >= rope[0]) & (vals <= rope[1])).sum(axis=1)
            assert np.array_equal(got["rope_share"], inside / S) and np.array_equal(got["rope_share"], (S - nb[3] - na[4]) / S), name
            xs = np.sort(vals, axis=1)
            for c, mm in enumerate(counts):
                win = np.array([((xs[i, j:j + mm] >= rope[0]) & (xs[i, j:j + mm] <= rope[1])).sum() for i, j in enumerate(ref["hdi_start"][c])])
                assert np.array_equal(got["rope_share_hdi"][c], win / mm), (name, mm)
            assert np.array_equal(got["rope_share_hdi"][2], got["rope_share"]) and 0 < inside.sum() < inside.size * S, name
    finally:
        fit.close()
