"""s4b_predict_quantiles on the device (stan4bart_amd/csrc/dev_quantile.inc: k_predict_values<staged>, k_predict_values<global>, k_row_quantiles) against
numpy on the full pooled matrix (tests/quantile_cases.py: the model and the derived bound).  Pooled draw counts 1, 2, 5, 13, 5 + 13 and 5 x 13 (one
beyond a wave); both routes, both links, a binary response, dense and ELL parts with ragged padding and another coefficient table per peer; bit-exact
anchors where h is an integer; permuted peers, a sampler pooled with itself, live and stored samplers; chunks of rows that are no multiple of the
tile; several rows per sort workgroup around its row count, one row per workgroup up to the LDS maximum and the refusal one handle beyond it; the
other refusals before any launch; determinism; the whole Python interface live and from stored samplers; one larger shape with the device memory of
the call against DESIGN.md 5.7's formula.

The chains are those of tests/test_gpu_predict_summary.py (n = 400, T <= 25, a dozen iterations); samplers with fewer draws are stored samplers
rebuilt from states exported while the chain ran.  The BART fits of the reference are computed once per sampler."""
import ctypes as C
import struct

import numpy as np
import pytest

import quantile_cases as qc
import readout_cases as rc
import summary_cases as sc
from conftest import make_sampler

pytestmark = pytest.mark.gpu
POOLS = {1: (1,), 2: (2,), 5: (5,), 13: (13,), 18: (5, 13), 65: (13,) * 5}          # pooled draws -> the stored samplers pooled, the first takes the call
PROBS = (0.025, 0.5, 0.975, 0.0, 1.0, 0.5, 1.0 / 3.0)


def _report(line):
    print(line)


class Chain:
    """One chain on the device: the live sampler (13 draws) and stored samplers holding its first 1, 2, 5 and 13 draws; hard rows of its rules filled
    up with new rows; predict_bart of every sampler at those rows."""

    def __init__(self, lib, args, steps=(1, 1, 3, 8), rows=2200):
        from stan4bart_amd.abi import StoredSampler
        assert args.keep_trees and args.iter - args.warmup == sum(steps)
        self.args, self.live, self.stored, kept = args, make_sampler(lib, "s4b_", args), {}, 0
        try:
            if args.warmup:
                self.live.run(args.warmup, True)
            self.live.disengage_adaptation()
            for more in steps:
                self.live.run(more, False)
                kept += more
                self.stored[kept] = StoredSampler(lib, "s4b_", self.live.export_bart_state())
            self.draws = kept
            self.range = self.live.get_bart_data_range()
            hard, _ = rc.predict_case_rows("summary", args, dict(kept_trees=self.live.get_kept_trees()), 0)
            self.x = np.asfortranarray(np.vstack([hard, rc.new_rows(args.x_bart, max(1, rows - len(hard)), seed=3)]))
            self.bart = {S: st.predict_bart(self.x) for S, st in self.stored.items()}
        except Exception:
            self.close()
            raise

    def close(self):
        for st in self.stored.values():
            st.free()
        self.live.free()


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


def _inputs(chain, pool, rows, M=0, E=0, offset=False, seed=0):
    """The arguments of a pooled call over the first `rows` rows and the model's `parts`: the row side (dense, ELL entries, offset) is shared, every
    pooled sampler gets a coefficient table of its own."""
    x = np.asfortranarray(chain.x[:rows])
    shared = sc.linear_parts(rows, pool[0], M, E, seed=seed)
    tables = [shared] + [sc.linear_parts(rows, S, M, E, seed=seed + 100 + j) for j, S in enumerate(pool[1:])]
    off = 1e3 * float(chain.range[1] - chain.range[0]) * np.random.default_rng(seed).uniform(-1.0, 1.0, rows) if offset else None
    kw = dict(offset=off, peers=[chain.stored[S] for S in pool[1:]], **shared)
    if M:
        kw["peer_dense_coef"] = [t["dense_coef"] for t in tables[1:]]
    if E:
        kw["peer_ell_coef"] = [t["ell_coef"] for t in tables[1:]]
    parts = [dict(bart=chain.bart[S][:rows], dense_coef=t.get("dense_coef"), ell_coef=t.get("ell_coef")) for S, t in zip(pool, tables)]
    row_side = dict(offset=off, dense=shared.get("dense"), ell_index=shared.get("ell_index"), ell_value=shared.get("ell_value"))
    return x, kw, parts, row_side


_REF = {}


def _case(chain, pool, rows, what, probs=PROBS, link=0, M=0, E=0, offset=False, seed=0, **call):
    """One pooled call against the model; the reference of a case is computed once and shared by the routes."""
    x, kw, parts, row_side = _inputs(chain, pool, rows, M, E, offset, seed)
    got = chain.stored[pool[0]].predict_quantiles(x, probs, link=link, **kw, **call)
    S = sum(pool)
    assert got["draws"] == S and got["info"]["draws"] == S and got["info"]["launches"] == 2 * got["info"]["chunks"]
    key = (id(chain), pool, rows, tuple(probs), link, M, E, offset, seed)
    if key not in _REF:
        _REF[key] = qc.model(parts, probs, link=link, **row_side)
    ref, bd, v, _ = _REF[key]
    qc.assert_quantiles(got, ref, bd, what, _report)
    return got, v, (x, kw)


@pytest.mark.parametrize("S", sorted(POOLS))
def test_pooled_draw_counts_against_the_model_on_both_routes(gauss, S):
    pool = POOLS[S]
    rows = 1024 + 37          # the hard rows (on, next to and far outside the cut points) and more: two tiles of the value kernel
    res = {}
    for route in ("staged", "global"):
        res[route], *_ = _case(gauss, pool, rows, f"S {S} {route}", M=2, E=2, offset=True, seed=S, route=route)
        info = res[route]["info"]
        sp = 1 << (S - 1).bit_length()
        assert info["route"] == (1 if route == "staged" else 2) and info["padded_draws"] == sp and info["rows_per_sort"] == 4096 // sp
        assert info["rows_per_chunk"] == rows and info["chunks"] == 1
    assert np.array_equal(res["staged"]["quantiles"], res["global"]["quantiles"]), "the two routes differ"
    q = res["staged"]["quantiles"]
    assert np.all(q[3] <= q[0]) and np.all(q[0] <= q[1]) and np.all(q[1] <= q[2]) and np.all(q[2] <= q[4]) and np.array_equal(q[1], q[5])
    if len(pool) > 1:          # every peer's own table reached its draws: the model with the first table for all is another answer
        _, kw, parts, row_side = _inputs(gauss, pool, rows, 2, 2, True, S)
        same = [dict(p, dense_coef=np.resize(parts[0]["dense_coef"], p["dense_coef"].shape), ell_coef=np.resize(parts[0]["ell_coef"], p["ell_coef"].shape))
                for p in parts]
        other, bd, *_ = qc.model(same, PROBS, **row_side)
        assert qc.bound_ratio(q, other, bd) > 1e6, "the peers' coefficient tables do not matter: the case tests no per-peer table"


@pytest.mark.parametrize("M,E", [(0, 0), (17, 0), (0, 3), (17, 3)])
def test_linear_parts_with_ragged_padding(gauss, M, E):
    for offset in (False, True):
        _, _, (x, kw) = _case(gauss, POOLS[18], 1024 + 5, f"M {M} E {E} offset {offset}", M=M, E=E, offset=offset, seed=M + E)
    if E:
        ix = kw["ell_index"]
        assert (ix == -1).any() and (ix == 0).any() and (ix == 6).any() and len({int(n) for n in (ix >= 0).sum(axis=1)}) > 1, "the padding is not ragged"


def test_links_and_binary_response(gauss, binary):
    assert binary.args.is_binary and not gauss.args.is_binary
    for chain, name in ((binary, "binary"), (gauss, "gauss")):
        for link in (1, 0):
            res = {}
            for route in ("staged", "global"):
                res[route], *_ = _case(chain, POOLS[18], 300, f"{name} link {link} {route}", link=link, M=2, E=1, seed=link, route=route)
            assert np.array_equal(res["staged"]["quantiles"], res["global"]["quantiles"])
            _case(chain, POOLS[5], 300, f"{name} link {link}, trees alone", link=link)
            if link:
                assert np.all((res["staged"]["quantiles"] >= 0) & (res["staged"]["quantiles"] <= 1))


@pytest.mark.parametrize("S", sorted(POOLS))
def test_integer_h_returns_the_order_statistic_bit_for_bit(gauss, S):
    """Link 0, no linear part: v is predict_bart's value, and a prob with an integer h = p (S - 1) returns one of them unchanged."""
    pool, rows = POOLS[S], 700
    probs = [0.0, 1.0] + ([0.5] if S % 2 else []) + ([0.25, 0.75] if S in (5, 13, 65) else []) + ([0.3, 0.9999] if S == 1 else [])
    xs = np.sort(np.concatenate([gauss.bart[s][:rows] for s in pool], axis=1), axis=1)
    for route in ("staged", "global"):
        got, *_ = _case(gauss, pool, rows, f"anchors S {S} {route}", probs=probs, route=route)
        for j, p in enumerate(probs):
            h = p * (S - 1)
            if S > 1:
                assert h == int(h), (p, S)
            assert np.array_equal(got["quantiles"][j], xs[:, int(h)]), f"S {S}, p {p}: not the order statistic {int(h)}"
    if S == 1:
        assert np.array_equal(got["quantiles"], np.repeat(gauss.bart[1][:rows].T, len(probs), axis=0)), "one draw: every quantile is the column"


def test_pooling_order_self_pooling_and_live_samplers(gauss):
    rows = 500
    a, _, (x, kw) = _case(gauss, (2, 5, 13), rows, "pool 2 + 5 + 13", M=1, E=2, offset=True, seed=3)
    # the same samplers with their tables in another order: the same multiset of values per row, the same bits
    peers, pd, pe = kw["peers"], kw["peer_dense_coef"], kw["peer_ell_coef"]
    rest = {k: v for k, v in kw.items() if k not in ("peers", "peer_dense_coef", "peer_ell_coef", "dense_coef", "ell_coef")}
    b = gauss.stored[13].predict_quantiles(x, PROBS, peers=[gauss.stored[2], peers[0]], dense_coef=pd[1], ell_coef=pe[1],
                                           peer_dense_coef=[kw["dense_coef"], pd[0]], peer_ell_coef=[kw["ell_coef"], pe[0]], **rest)
    assert b["draws"] == 20 and np.array_equal(a["quantiles"], b["quantiles"]), "permuting the pool changes the bits"
    # the live sampler holds the kept trees of stored[13]: as the caller and as a peer
    c = gauss.live.predict_quantiles(x, PROBS, peers=[gauss.stored[2], peers[0]], dense_coef=pd[1], ell_coef=pe[1],
                                     peer_dense_coef=[kw["dense_coef"], pd[0]], peer_ell_coef=[kw["ell_coef"], pe[0]], **rest)
    d = gauss.stored[2].predict_quantiles(x, PROBS, peers=[peers[0], gauss.live], dense_coef=kw["dense_coef"], ell_coef=kw["ell_coef"],
                                          peer_dense_coef=pd, peer_ell_coef=pe, **rest)
    assert np.array_equal(c["quantiles"], a["quantiles"]) and np.array_equal(d["quantiles"], a["quantiles"]) and c["info"] == b["info"]
    # a sampler pooled with itself (a handle twice, the caller included): all ties — minimum, median and maximum are those of the sampler alone
    for S in (5, 13):
        alone = gauss.stored[S].predict_quantiles(x, [0.0, 0.5, 1.0])
        for times in (2, 3):
            again = gauss.stored[S].predict_quantiles(x, [0.0, 0.5, 1.0], peers=[gauss.stored[S]] * (times - 1))
            assert again["draws"] == times * S and np.array_equal(again["quantiles"], alone["quantiles"]), (S, times)


def test_chunks_of_rows(gauss):
    pool, S = POOLS[18], 18
    for rows, C, chunks in ((130, 64, 3), (2 * 1024 + 1, 1024 + 64, 2)):
        whole, _, (x, kw) = _case(gauss, pool, rows, f"{rows} rows in one chunk", M=1, E=1, offset=True, seed=rows)
        assert whole["info"]["chunks"] == 1 and whole["info"]["rows_per_chunk"] == rows and whole["info"]["launches"] == 2
        for route in ("staged", "global"):
            got = gauss.stored[pool[0]].predict_quantiles(x, PROBS, scratch_bytes=8 * S * C + 8 * S * 63, route=route, **kw)          # (rounded down to 64 rows)
            info = got["info"]
            assert (info["rows_per_chunk"], info["chunks"], info["launches"]) == (C, chunks, 2 * chunks), info
            assert rows - (chunks - 1) * C in (2, 961) and np.array_equal(got["quantiles"], whole["quantiles"]), f"{rows} rows in chunks of {C}: other bits"
    tiny = gauss.stored[pool[0]].predict_quantiles(x[:130], PROBS, scratch_bytes=1, **{k: (v[:130] if k in ("offset", "dense", "ell_index", "ell_value") else v) for k, v in kw.items()})
    assert tiny["info"]["rows_per_chunk"] == 64 and tiny["info"]["chunks"] == 3          # at least 64 rows per chunk


@pytest.mark.parametrize("rows", [127, 128, 129])
def test_rows_around_a_sort_workgroup(gauss, rows):
    got, *_ = _case(gauss, POOLS[18], rows, f"{rows} rows, 128 per sort workgroup", M=1, seed=rows)
    assert got["info"]["rows_per_sort"] == 128 and got["info"]["padded_draws"] == 32


@pytest.mark.parametrize("times,rows", [(316, 70), (1260, 3)])
def test_one_row_per_sort_workgroup_up_to_the_lds_maximum(gauss, times, rows):
    S = 13 * times
    x = np.asfortranarray(gauss.x[:rows])
    probs = (0.0, 0.025, 0.5, 0.975, 1.0)
    got = gauss.stored[13].predict_quantiles(x, probs, peers=[gauss.stored[13]] * (times - 1))
    sp = 1 << (S - 1).bit_length()
    assert got["draws"] == S and got["info"]["padded_draws"] == sp and got["info"]["rows_per_sort"] == 1 and sp == (8192 if times == 316 else 16384)
    v = np.tile(gauss.bart[13][:rows], (1, times))
    qc.assert_quantiles(got, qc.type7(v, probs).astype(np.float64), qc.bound(v, np.zeros_like(v), len(probs)), f"S {S}", _report)
    assert np.array_equal(got["quantiles"][0], v.min(axis=1)) and np.array_equal(got["quantiles"][4], v.max(axis=1))


def test_one_handle_beyond_the_largest_pool_is_refused(gauss):
    x = np.asfortranarray(gauss.x[:3])
    before = gauss.live.get_counters()
    with pytest.raises(RuntimeError, match="16393 pooled draws, at most 16384"):
        gauss.live.predict_quantiles(x, [0.5], peers=[gauss.stored[13]] * 1260)
    assert not any(gauss.live.quantile_info.values()) and np.array_equal(gauss.live.get_counters(), before)


def test_refusals_come_before_any_launch(hip_lib, gauss, binary):
    from stan4bart_amd.abi import QuantileIn, QuantileOut, Sampler
    rows, S = 50, 13
    x = np.asfortranarray(gauss.x[:rows])
    live = gauss.live
    parts = sc.linear_parts(rows, S, 1, 2)
    peer = sc.linear_parts(rows, 5, 1, 2, seed=1)

    def refused(match, probs=(0.5,), samplers=None, **kw):
        before = live.get_counters()
        for smp in samplers or (live, gauss.stored[S]):
            with pytest.raises(RuntimeError, match=match):
                smp.predict_quantiles(x, probs, **kw)
            assert smp.quantile_info["launches"] == 0 and not any(smp.quantile_info.values())
        assert np.array_equal(live.get_counters(), before), "a refused call launched something"
    assert binary.args.n_trees != gauss.args.n_trees
    refused("peer 1 has 11 trees per draw, the sampler 25", peers=[gauss.stored[5], binary.stored[5]])
    refused(r"prob -0\.1\d* outside \[0, 1\]", probs=(0.5, -0.1))
    refused(r"prob 1\.5\d* outside \[0, 1\]", probs=(1.5,))
    refused(r"prob -?nan outside \[0, 1\]", probs=(0.1, np.nan, 0.9))
    refused("between 1 and 16 probs per call, not 0", probs=())
    refused("between 1 and 16 probs per call, not 17", probs=np.linspace(0, 1, 17))
    refused("n_dense > 0 needs peer_dense_coef", peers=[gauss.stored[5]], dense=parts["dense"], dense_coef=parts["dense_coef"])
    refused("n_ell > 0 needs peer_ell_coef", peers=[gauss.stored[5]], peer_dense_coef=[peer["dense_coef"]], **parts)
    refused("link must be 0", link=2)
    refused("negative scratch_bytes", scratch_bytes=-1)
    # a peer of the same shape trained on other rows: other cut points
    other = make_sampler(hip_lib, "s4b_", rc._friedman(n=410, T=25, warmup=2, iter=3, ranef=False))
    fresh = make_sampler(hip_lib, "s4b_", gauss.args)          # keep_trees, but no sampling run yet
    try:
        other.run(2, True)
        other.disengage_adaptation()
        other.run(1, False)
        refused(r"peer 0 has other cut points of predictor \d+", peers=[other])
        refused("peer 1 holds no kept draws", peers=[gauss.stored[5], fresh])
        refused("the sampler holds no kept draws", samplers=(fresh,))
    finally:
        other.free()
        fresh.free()
    # a weight vector (the Python method offers none: the structure is filled here)
    rows_in, keep, _, _ = Sampler._summary_in(S, x, None, None, None, None, None, None, 0, np.ones((1, rows)), "auto", 0, 0)
    pr, buf = np.array([0.5]), np.zeros(rows)
    arg = QuantileIn(rows=rows_in, n_probs=1, probs=pr.ctypes.data_as(C.POINTER(C.c_double)))
    out = QuantileOut(quantiles=buf.ctypes.data_as(C.POINTER(C.c_double)))
    before = live.get_counters()
    assert hip_lib.s4b_predict_quantiles(live._h, C.byref(arg), C.byref(out)) == 1
    assert "n_weights must be 0" in hip_lib.s4b_last_error().decode() and not any(out.info) and np.array_equal(live.get_counters(), before)
    ok = live.predict_quantiles(x, [0.5], peers=[gauss.stored[5]], peer_dense_coef=[peer["dense_coef"]], peer_ell_coef=[peer["ell_coef"]], **parts)
    assert ok["info"]["launches"] == 2 and live.get_counters()[2] == before[2] + 2 and ok["draws"] == 18


def test_same_call_twice_is_bit_identical(gauss):
    for route in ("staged", "global"):
        a, _, (x, kw) = _case(gauss, POOLS[65], 2 * 1024 + 1, f"determinism {route}", link=1, M=3, E=3, offset=True, route=route, scratch_bytes=8 * 65 * 1088)
        b = gauss.stored[13].predict_quantiles(x, PROBS, link=1, route=route, scratch_bytes=8 * 65 * 1088, **kw)
        assert a["info"]["chunks"] == 2 and np.array_equal(a["quantiles"], b["quantiles"]), route


def test_whole_interface_live_and_stored(hip_lib):
    """Stan4bartFit.predict_quantiles against the model over fit.predict(..., combine_chains=False) of the same seed and against np.quantile: two
    chains, fixed effects, a random slope term, unseen levels; once from the live samplers, once after attach_stored_samplers."""
    from stan4bart_amd import GroupTerm, generate_friedman_data
    from stan4bart_amd.abi import Sampler
    from stan4bart_amd.generics import combine_chains_f, stan4bart
    d = generate_friedman_data(120, ranef=True, causal=True, p=10)
    x = d["x"]
    xb, X = x[:, [j for j in range(10) if j != 3]], np.column_stack([x[:, 3], d["z"]])
    groups = [GroupTerm(d["g1"], x[:, 3], "g.1"), GroupTerm(d["g2"], None, "g.2")]
    fit = stan4bart(d["y"], xb, X=X, groups=groups, chains=2, seed=99, iter=14, warmup=6, bart_args={"n.trees": 9, "keepTrees": True},
                    make_sampler=lambda a, st: Sampler(hip_lib, "s4b_", a, st))
    try:
        m = 45
        g = np.random.default_rng(11)
        lev1 = np.asarray(d["g1"])[:m].copy()
        lev1[::4] = 6 + (np.arange(len(lev1[::4])) % 2)          # g.1 has five levels: 6 and 7 are unseen
        new = [GroupTerm(lev1, x[:m, 3] + 0.25, "g.1"), GroupTerm(np.asarray(d["g2"])[:m], None, "g.2")]
        xb_new, X_new, off = rc.new_rows(xb, m, seed=4), X[:m] + g.normal(size=(m, 2)), g.normal(size=m)
        full = fit.predict(x_bart=xb_new, X=X_new, groups=new, offset=off, combine_chains=False, seed=7)          # [rows, iter, chain]
        assert full.shape == (m, 8, 2)
        # the bound of a value: the model over the builder's own tables, once for the device and once more for the arithmetic of fit.predict itself
        ix, val, coef = fit._ell_random(new, True, np.random.default_rng(7))
        assert ix.max() >= fit.stan[fit._rows("b.")].shape[0], "no unseen level reached the table"
        beta = fit.stan[fit._rows("beta.")]
        bart = np.concatenate([s.predict_bart(xb_new) for s in fit.samplers], axis=1)
        mref, mbound = sc.model(bart, off, X_new - fit.X_means, np.concatenate([beta[:, :, c].T for c in range(2)]), ix, val, np.concatenate(coef))
        flat = combine_chains_f(full)
        assert sc.bound_ratio(flat, mref["v"], mbound["v"]) <= sc.BOUND_FACTOR, "fit.predict and the model over the ELL table describe different draws"
        probs = (0.025, 0.5, 0.975, 0.2)
        ref, bd = qc.type7(flat, probs).astype(np.float64), qc.bound(flat, 2.0 * mbound["v"], len(probs))

        def check(what):
            got = fit.predict_quantiles(x_bart=xb_new, X=X_new, groups=new, offset=off, probs=probs, seed=7)
            assert got["draws"] == 16 and got["quantiles"].shape == (4, m) and np.array_equal(got["probs"], probs)
            r = qc.bound_ratio(got["quantiles"], ref, bd)
            print(f"whole interface, {what}: max |device - model over fit.predict| / bound = {r:.3g}")
            assert r <= qc.BOUND_FACTOR, r
            np.testing.assert_allclose(got["quantiles"], np.quantile(flat, probs, axis=1), rtol=1e-9)
            default = fit.predict_quantiles(x_bart=xb_new, type="indiv.bart")
            assert np.array_equal(default["probs"], (0.025, 0.5, 0.975))
            np.testing.assert_allclose(default["quantiles"], np.quantile(bart, (0.025, 0.5, 0.975), axis=1), rtol=1e-12)
            return got
        a = check("live samplers")
        fit.attach_stored_samplers(fit.export_bart_states(), lib=hip_lib)
        b = check("stored samplers")
        assert np.array_equal(a["quantiles"], b["quantiles"])
    finally:
        fit.close()


def test_larger_shape_and_device_memory(hip_lib):
    rows, S, T = 200000, 8, 5
    args = rc.PREDICT_CASES["cap-exact"][0]()
    assert args.n_trees == T and args.iter - args.warmup == S
    chain = Chain(hip_lib, args, steps=(S,), rows=rows)
    try:
        assert len(chain.x) == rows
        probs = (0.025, 0.5, 0.975)
        got, *_ = _case(chain, (S,), rows, "200000 rows", probs=probs, M=1, E=1, offset=True, scratch_bytes=1 << 20)
        nodes = struct.unpack_from("<Q", chain.live.export_bart_state(), 28)[0]
        info = got["info"]
        assert info["rows_per_chunk"] * 8 * S <= 1 << 20 and info["rows_per_chunk"] == 16384 and info["chunks"] == -(-rows // 16384)
        want = qc.device_bytes_formula(args.x_bart.shape[1], rows, nodes, S, T, True, 1, 1, 7, info["rows_per_chunk"], len(probs))
        print(f"device memory of the call: {info['device_bytes']} bytes, formula {want}; a draws matrix would add {8 * rows * S - 8 * info['rows_per_chunk'] * S}")
        assert info["device_bytes"] == want
    finally:
        chain.close()
