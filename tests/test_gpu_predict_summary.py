"""s4b_predict_summary on the device (stan4bart_amd/csrc/dev_summary.inc: k_predict_summary<staged>, k_predict_summary<global>, k_summary_fold) against
numpy on the full matrix (tests/summary_cases.py: the model, the derived bounds, the inputs).  Shapes are stated in the kernel's own constants,
read from the `info` words of a call: rows around one tile and into a workgroup's second tile; 1, 2 and an odd number of draws (the two staging
buffers' parity); the largest draw below, exactly at and one node beyond the staging buffer (route asserted from `info`, both routes bit-equal);
dense and ELL parts with ragged padding; both links, a binary response; 1, 3 and 8 weight vectors; determinism; refusals before any launch; the
whole Python interface live and from stored samplers; one larger shape with the device memory of the call against DESIGN.md's formula.

The chains are tiny (n = 400, T <= 25, a dozen iterations); samplers with fewer draws are stored samplers rebuilt from states exported while the
chain ran, so one chain serves every number of draws."""
import os
import re
import struct

import numpy as np
import pytest

import readout_cases as rc
import summary_cases as sc
from conftest import make_sampler

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _report(line):
    print(line)


class Chain:
    """One chain on the device: the live sampler (all draws) and stored samplers holding its first 1, 2, 5 and all draws; hard rows of its rules
    filled up with new rows."""

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
            self.n_hard = len(hard)
            self.x = np.asfortranarray(np.vstack([hard, rc.new_rows(args.x_bart, max(1, rows - len(hard)), seed=3)]))
            self.bart = {S: st.predict_bart(self.x) for S, st in self.stored.items()}          # the reference's BART fits, once per sampler
            for S, b in self.bart.items():
                assert b.shape == (len(self.x), S) and np.array_equal(b, self.bart[self.draws][:, :S])
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


@pytest.fixture(scope="module")
def deep(hip_lib):
    c = Chain(hip_lib, rc.PREDICT_CASES["deep"][0](), steps=(1, 1, 2), rows=1100)
    yield c
    c.close()


def _tile(chain):
    info = chain.stored[1].predict_summary(chain.x[:1])["info"]
    src = open(os.path.join(ROOT, "stan4bart_amd", "csrc", "dev_summary.inc")).read()
    assert info["rows_per_tile"] == int(re.search(r"constexpr int PS_BLOCK = (\d+);", src).group(1))
    return info["rows_per_tile"]


def _stage_cap():
    src = open(os.path.join(ROOT, "stan4bart_amd", "csrc", "dev_summary.inc")).read()
    return int(re.search(r"constexpr int PS_STAGE_NODES = (\d+);", src).group(1))


def _case(chain, S, rows, what, link=0, M=0, E=0, G=1, offset=False, seed=0, **kw):
    """One call on the stored sampler with S draws over the first `rows` rows against the model: (result, reference, bounds, inputs)."""
    smp, x = chain.stored[S], np.asfortranarray(chain.x[:rows])
    parts = sc.linear_parts(rows, S, M, E, seed=seed)
    w = sc.weight_vectors(rows, G, seed=seed) if G else None
    off = None
    if offset:          # an offset of 1e3 response ranges
        off = 1e3 * float(chain.range[1] - chain.range[0]) * np.random.default_rng(seed).uniform(-1.0, 1.0, rows)
    got = smp.predict_summary(x, offset=off, link=link, weights=w, **parts, **kw)
    assert got["draws"] == S and got["info"]["launches"] == (2 if G else 1)
    ref, bound = sc.model(chain.bart[S][:rows], off, link=link, weights=w, **parts)
    sc.assert_summary(got, ref, bound, what, _report)
    return got, ref, bound, dict(x=x, offset=off, link=link, weights=w, **parts)


def test_rows_around_a_tile_and_a_second_tile(gauss):
    tile = _tile(gauss)
    assert len(gauss.x) >= 2 * tile + 1 and gauss.n_hard < tile - 1
    for rows, kw in ((1, {}), (tile - 1, {}), (tile, {}), (tile + 1, {}), (2 * tile + 1, dict(max_workgroups=2))):
        for route in ("staged", "global"):
            got, *_ = _case(gauss, 5, rows, f"rows {rows} {route}", M=1, E=1, G=3, route=route, **kw)
            want = min(-(-rows // tile), kw.get("max_workgroups", 1 << 30))
            assert got["info"]["workgroups"] == want and got["info"]["route"] == (1 if route == "staged" else 2)
    # 2 workgroups x tile + 1 rows: workgroup 0 comes round to a second tile, where its per-draw partials accumulate
    assert got["info"]["workgroups"] == 2 and got["info"]["workgroups"] * tile + 1 == 2 * tile + 1


@pytest.mark.parametrize("S", [1, 2, 5])
def test_draws_one_two_and_odd(gauss, S):
    tile = _tile(gauss)
    rows = tile + 37          # the hard rows (on, next to and far outside the cut points) and more, two workgroups
    assert gauss.n_hard < rows and np.isinf(gauss.x[:rows]).any()
    res = {}
    for route in ("staged", "global"):
        res[route], *_ = _case(gauss, S, rows, f"S {S} {route}", M=2, E=2, G=3, route=route)
    for key in ("mean", "m2", "average"):
        assert np.array_equal(res["staged"][key], res["global"][key]), key
    if S == 1:
        x = np.asfortranarray(gauss.x[:rows])
        hot = np.zeros((2, rows))
        hot[0, 5], hot[1, rows - 1] = 1.0, 1.0
        for route in ("staged", "global"):
            got = gauss.stored[1].predict_summary(x, weights=hot, route=route)
            assert not got["m2"].any(), "one draw: m2 must be exactly zero"
            assert np.array_equal(got["mean"], gauss.bart[1][:rows, 0]), "one draw, no linear part, link 0: the mean is predict_bart's column"
            assert got["average"][0, 0] == gauss.bart[1][5, 0] and got["average"][0, 1] == gauss.bart[1][rows - 1, 0]


@pytest.mark.parametrize("which", ["deep", "gauss"])
def test_routes_around_the_staging_buffer(which, deep, gauss):
    chain = deep if which == "deep" else gauss
    S = chain.draws
    x = np.asfortranarray(chain.x[:1100])
    auto = chain.stored[S].predict_summary(x)
    largest, cap = auto["info"]["largest_draw_nodes"], _stage_cap()
    if which == "deep":
        assert chain.args.node_capacity == 1024 and rc.nodes_per_tree(chain.live.get_kept_trees()).max() > 128
    else:
        assert largest + 1 <= cap
    ref, bound = sc.model(chain.bart[S][:1100])
    seen = set()
    for knob in (largest + 1, largest, largest - 1):          # the largest draw below the buffer, filling it exactly, one node beyond it
        got = chain.stored[S].predict_summary(x, stage_nodes=knob)
        want = 1 if largest <= min(knob, cap) else 2
        info = got["info"]
        assert info["route"] == want and info["largest_draw_nodes"] == largest, (knob, info)
        if want == 1:
            assert info["staging_nodes"] == min(knob, cap) and info["staging_bytes"] == 16 * info["staging_nodes"] + 4 * chain.args.n_trees
        else:
            assert info["staging_nodes"] == 0 and info["staging_bytes"] == 0
        seen.add(want)
        sc.assert_summary(got, ref, bound, f"{which} stage_nodes {knob}", _report)
        assert np.array_equal(got["mean"], auto["mean"]) and np.array_equal(got["m2"], auto["m2"]), "the two routes differ"
    forced = chain.stored[S].predict_summary(x, route="global")
    assert forced["info"]["route"] == 2 and np.array_equal(forced["mean"], auto["mean"]) and np.array_equal(forced["m2"], auto["m2"])
    assert 2 in seen and (which == "deep" or seen == {1, 2})
    live = chain.live.predict_summary(x)          # the live sampler holds the same kept trees
    assert np.array_equal(live["mean"], auto["mean"]) and live["info"]["route"] == auto["info"]["route"]


@pytest.mark.parametrize("M,E", [(0, 0), (1, 0), (17, 0), (0, 1), (0, 3), (17, 3)])
def test_linear_parts(gauss, M, E):
    rows = _tile(gauss) + 5
    for offset in (False, True):
        got, ref, bound, inp = _case(gauss, 5, rows, f"M {M} E {E} offset {offset}", M=M, E=E, G=1, offset=offset, seed=M + E)
    if E:
        ix = inp["ell_index"]
        assert (ix == -1).any() and (ix == 0).any() and (ix == 6).any()
        if E > 1:
            assert len({int(n) for n in (ix >= 0).sum(axis=1)}) > 1, "the padding is not ragged"


def test_links_and_binary_response(gauss, binary):
    """Both links on both responses.  With one draw and no linear part the mean IS Phi(predict_bart): the accuracy constant of erfc is measured here."""
    rows = _tile(binary) + 9
    for chain, name in ((binary, "binary"), (gauss, "gauss")):
        for link in (1, 0):
            _case(chain, 5, rows, f"{name} link {link}", link=link, M=2, E=1, G=3, seed=link)
            _case(chain, 5, rows, f"{name} link {link}, trees alone", link=link, G=1)
    assert binary.args.is_binary
    worst = 0.0
    for chain in (binary, gauss):
        z = chain.bart[1][:rows, 0]
        got = chain.stored[1].predict_summary(np.asfortranarray(chain.x[:rows]), link=1)
        assert not got["m2"].any()
        err = np.abs(got["mean"].astype(np.longdouble) - sc.phi_cdf(z).astype(np.longdouble)).astype(np.float64) / sc.U
        worst = max(worst, float(err.max()))
    print(f"erfc accuracy: largest |device Phi - math.erfc Phi| / u over {2 * rows} arguments = {worst:.3f} (ERFC_C = {sc.ERFC_C:g})")
    assert worst <= sc.ERFC_C, (worst, sc.ERFC_C)
    assert np.all((got["mean"] >= 0) & (got["mean"] <= 1))


@pytest.mark.parametrize("G", [1, 3, 8])
def test_weight_vectors(gauss, G):
    rows = _tile(gauss) + 11
    got, ref, bound, inp = _case(gauss, 13, rows, f"G {G}", M=1, G=G, seed=G)
    w = inp["weights"]
    assert got["average"].shape == (13, G) and w[0].sum() == pytest.approx(1.0)
    if G >= 3:
        assert (w[2] == 0).any() and (w[2] < 0).any() and set(np.unique(w[1] * (w[1] > 0).sum())) <= {0.0, 1.0}


def test_no_weights_no_fold(gauss):
    got, *_ = _case(gauss, 5, 300, "G 0", M=1, G=0)
    assert got["average"].shape == (5, 0) and got["info"]["launches"] == 1


def test_same_call_twice_is_bit_identical(gauss):
    rows = 2 * _tile(gauss) + 1
    for route in ("staged", "global"):
        a, _, _, inp = _case(gauss, 13, rows, f"determinism {route}", link=1, M=3, E=3, G=8, offset=True, route=route, max_workgroups=2)
        x = inp.pop("x")
        b = gauss.stored[13].predict_summary(x, route=route, max_workgroups=2, **inp)
        for key in ("mean", "m2", "average"):
            assert np.array_equal(a[key], b[key]), (route, key)


def test_refusals_come_before_any_launch(gauss):
    rows, S, q = 50, 13, 7
    x = np.asfortranarray(gauss.x[:rows])
    parts = sc.linear_parts(rows, S, 1, 2, q=q)
    live = gauss.live

    def refused(match, **kw):
        args = dict(parts)
        args.update(kw)
        xx = args.pop("x", x)
        before = live.get_counters()
        for smp in (live, gauss.stored[S]):
            with pytest.raises(RuntimeError, match=match):
                smp.predict_summary(xx, **args)
            assert smp.summary_info["launches"] == 0 and smp.summary_info["route"] == 0
        assert np.array_equal(live.get_counters(), before), "a refused call launched something"
    for bad, match in ((q, r"ell_index 7 outside \[-1, 7\)"), (-2, r"ell_index -2 outside")):
        ix = parts["ell_index"].copy()
        ix[rows - 1, 1] = bad
        refused(match, ell_index=ix)
    refused("between 0 and 8 weight vectors, not 9", weights=np.ones((9, rows)))
    refused("link must be 0", link=2)
    refused("at least one row", x=np.zeros((0, x.shape[1])), dense=None, dense_coef=None, ell_index=None, ell_value=None, ell_coef=None)
    before = live.get_counters()
    ok = live.predict_summary(x, weights=np.ones((1, rows)), **parts)
    assert ok["info"]["launches"] == 2 and live.get_counters()[2] == before[2] + 2


def test_whole_interface_live_and_stored(hip_lib):
    """Stan4bartFit.predict_summary against numpy on fit.predict(..., combine_chains=False) of the same seed: two chains, fixed effects, a random
    slope term, unseen levels; once from the live samplers, once after attach_stored_samplers."""
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
        w = sc.weight_vectors(m, 3)
        full = fit.predict(x_bart=xb_new, X=X_new, groups=new, offset=off, combine_chains=False, seed=7)          # [rows, iter, chain]
        assert full.shape == (m, 8, 2)
        # the bound of an entry: the model over the builder's own tables (its values are not the reference: fit.predict is), once for the device and
        # once more for the double-precision arithmetic of fit.predict itself
        ix, val, coef = fit._ell_random(new, True, np.random.default_rng(7))
        assert ix.max() >= fit.stan[fit._rows("b.")].shape[0], "no unseen level reached the table"
        beta = fit.stan[fit._rows("beta.")]
        bart = np.concatenate([s.predict_bart(xb_new) for s in fit.samplers], axis=1)
        mref, mbound = sc.model(bart, off, X_new - fit.X_means, np.concatenate([beta[:, :, c].T for c in range(2)]), ix, val, np.concatenate(coef))
        flat = combine_chains_f(full)
        assert sc.bound_ratio(flat, mref["v"], mbound["v"]) <= sc.BOUND_FACTOR, "fit.predict and the model over the ELL table describe different draws"
        ref, bound = sc.summarise(flat.astype(np.longdouble), 2.0 * mbound["v"], w)

        def check(what):
            got = fit.predict_summary(x_bart=xb_new, X=X_new, groups=new, offset=off, row_weights=w, seed=7)
            assert got["draws"] == 16 and got["average"].shape == (3, 16)
            split = fit.predict_summary(x_bart=xb_new, X=X_new, groups=new, offset=off, row_weights=w, seed=7, combine_chains=False)
            assert split["average"].shape == (3, 8, 2) and np.array_equal(combine_chains_f(split["average"]), got["average"])
            r = dict(mean=sc.bound_ratio(got["mean"], ref["mean"], bound["mean"]), m2=sc.bound_ratio(got["sd"] ** 2 * 15, ref["m2"], 2.0 * bound["m2"]),
                     average=sc.bound_ratio(got["average"].T, ref["average"], bound["average"]))
            print(f"whole interface, {what}: max |device - numpy on predict| / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
            assert max(r.values()) <= sc.BOUND_FACTOR, r
            np.testing.assert_allclose(got["sd"], np.std(flat, axis=1, ddof=1), rtol=1e-9)
            default = fit.predict_summary(x_bart=xb_new, type="indiv.bart")
            assert default["average"].shape == (1, 16)
            np.testing.assert_allclose(default["average"][0], bart.mean(axis=0), rtol=1e-12)
            return got
        a = check("live samplers")
        fit.attach_stored_samplers(fit.export_bart_states(), lib=hip_lib)
        b = check("stored samplers")
        for key in ("mean", "sd", "average"):
            assert np.array_equal(a[key], b[key]), key
    finally:
        fit.close()


def _device_bytes_formula(P, rows, nodes, S, T, offset, M, E, q, G, workgroups):
    """the device memory of one call (every allocation at least 16 bytes)."""
    sizes = [2 * P * rows, 24 * nodes, 8 * S * T, 16 * S, 8 * rows, 8 * rows]          # binned rows, nodes, tree starts, scales, mean, m2
    if offset:
        sizes.append(8 * rows)
    if M:
        sizes += [8 * rows * M, 8 * S * M]
    if E:
        sizes += [4 * rows * E, 8 * rows * E, 8 * S * q]
    if G:
        sizes += [8 * G * rows, 8 * workgroups * S * G, 8 * S * G]          # weights, the workgroups' partials, average
    return sum(max(16, t) for t in sizes)


def test_larger_shape_and_device_memory(hip_lib):
    rows, S, T = 200000, 8, 5
    args = rc.PREDICT_CASES["cap-exact"][0]()
    assert args.n_trees == T and args.iter - args.warmup == S
    chain = Chain(hip_lib, args, steps=(S,), rows=rows)
    try:
        assert len(chain.x) == rows
        got, ref, bound, inp = _case(chain, S, rows, "200000 rows", M=1, E=1, G=2, offset=True)
        state = chain.live.export_bart_state()
        nodes = struct.unpack_from("<Q", state, 28)[0]
        info = got["info"]
        assert info["workgroups"] == -(-rows // info["rows_per_tile"])
        want = _device_bytes_formula(args.x_bart.shape[1], rows, nodes, S, T, True, 1, 1, 7, 2, info["workgroups"])
        print(f"device memory of the call: {info['device_bytes']} bytes, formula {want}; a draws matrix would add {8 * rows * S}")
        assert info["device_bytes"] <= want < info["device_bytes"] + 8 * rows * S
    finally:
        chain.close()
