"""s4b_predict_curves (stan4bart_amd/csrc/readout_curves.inc over dev_readout.inc, dev_pd.inc, dev_quantile.inc, dev_groups.inc: k_curve_values<staged /
global, cancelling or not>, k_curve_rows, k_level_rows, k_row_quantiles) — the model, the bounds, the counts and the cases
shared by tests/test_predict_curves.py (CPU) and tests/test_gpu_predict_curves.py (GPU).

The model.  For every grid point g the rows get their column(s) `vars` overwritten (pd_cases.overwritten) and go through predict_bart of every pooled
sampler; the linear parts (at the rows' own values) are added in long double in summary_cases.model's order (contrast_cases.linear), Phi is
summary_cases.phi_cdf; v(i,g,k) so formed is centred, c = v_g - v_a, where an anchor a is given; then mean, m2 and type-7 quantiles along the draws
(summary_cases.summarise, quantile_cases.type7), and max, min and r = max - min across g.

Bound of c(i,g,k) (u = 2^-53; every comparison allows readout_cases.BOUND_FACTOR x the bound; no measured constant but summary_cases.ERFC_C):
  order_g   = (T + 2) u (F_g + 0.5) w + u |lo|  pd_cases' term of a T-term leaf sum added in another order than predict_bart's (binary response: w = 1,
              lo = 0, no + 0.5), F_g = sum_t |mu_t| at the overwritten row.
  no anchor   pd_cases' per-element bound: summary_cases' bound of v, ops u A (link 1: phi(z) (ops + 2) u A + ERFC_C u), plus order_g (link 1: phi(z) order_g).
  anchor, link 1   bound(v_g) + bound(v_a) + u |c|: both values as above, one rounding of the difference.  At the anchor both sides are exactly 0.
  anchor, link 0   the device forms w (s_g - s_a) over the affected trees alone: contrast_cases' bound of the cancelled form without linear parts,
              (A > 0) (order_g + order_a) + (A + 2) u w (G_g + G_a) + 3 u w (G_g + G_a), G the sum of |mu_t| over the A affected trees.
Bounds of the outputs: mean and m2 by summary_cases.summarise (k_level_rows runs k_contrast_reduce's two-pass arithmetic, which contrast_cases shows to
lie inside it), quantiles by quantile_cases.bound.  The range: |max_g a_g - max_g b_g| <= max_g |a_g - b_g|, so bound(r) = 2 max_g bound(c_g) + u |r|
(0 where all grid points are in one exact-tie class, below: r is then exactly 0 on both sides), carried through summarise and quantile_cases.bound like a value.

Counts.  Two grid points are in one EXACT-TIE CLASS of a (row, draw) when the row reaches the same leaf in every tree of the draw under both — which
equal bins on the varied predictors imply, and which makes the values bit-equal on the device (the same leaves added in the same order) and in the
model (predict_bart of the same leaves).  Within a class only the lowest index can win.  A point is a CERTAIN winner if it is the lowest of its class and
beats every point outside the class by more than the two bounds added; it is a POSSIBLE winner if it is the lowest of its class and no point outside
beats it by more than that.  certain[g] <= S p_max[g] <= possible[g] per (row, g), likewise p_min: nothing is left out, the slack is the count of
ambiguous draws.  ambiguity() is the share of (row, draw) pairs without a certain maximum or without a certain minimum: at most AMBIGUOUS_MAX in every
case, asserted on the CPU from the model alone, so the sandwich cannot go vacuous."""
import numpy as np

import contrast_cases as cc
import pd_cases as pc
import quantile_cases as qc
import readout_cases as rc
import summary_cases as sc
from readout_cases import BOUND_FACTOR, U, bound_ratio  # noqa: F401

LD = np.longdouble
AMBIGUOUS_MAX = 0.05
PROBS = (0.025, 0.5, 0.975, 0.0, 1.0)
PER_POINT = ("mean", "m2", "quantiles")


def chunk_rows(n_test, S, G, scratch_bytes=0, default=512 << 20):
    """The chunk-size rule restated: C = scratch / (8 S G) rounded down to a multiple of 64, at least 64, at most n_test."""
    scratch = min(scratch_bytes, default) if scratch_bytes > 0 else default
    return min(n_test, max(64, scratch // (8 * S * G) // 64 * 64))


def leaf_walk(trees, x, hit):
    """(F, Ga, sig) [rows x S]: sum |mu_t| over all trees, over the trees marked in `hit` [S x T], and a 64-bit signature of the leaves reached in all
    trees of the draw (a polynomial hash of the leaf entries: equal leaves give equal signatures; a collision of unequal ones is not to be expected)."""
    S, T = hit.shape
    F, Ga, sig = np.zeros((len(x), S)), np.zeros((len(x), S)), np.zeros((len(x), S), dtype=np.uint64)
    for a, _, pos in rc.walk_leaves(trees, x):
        mu = np.abs(trees["value"][pos])
        F[:, a // T] += mu
        if hit[a // T, a % T]:
            Ga[:, a // T] += mu
        sig[:, a // T] = sig[:, a // T] * np.uint64(0x9E3779B97F4A7C15) + pos.astype(np.uint64) + np.uint64(1)
    return F, Ga, sig


def model(parts, x, vars, grid, T, ranges, binary, anchor=None, link=0, probs=(), offset=None, dense=None, ell_index=None, ell_value=None):
    """`parts`: per pooled sampler, in pooling order, dict(predict_bart: rows -> [rows x draws], trees: get_kept_trees(), hit [draws x T]
    (pd_cases.affected of `vars`), dense_coef, ell_coef).  Returns (ref, bound, extra): dicts with c [rows x G x S], mean, m2 [rows x G], quantiles
    [Q x rows x G], r [rows x S], range_mean, range_m2 [rows], range_quantiles [Q x rows]; extra holds sig [rows x G x S]."""
    x = np.asarray(x, dtype=np.float64)
    rows = x.shape[0]
    grid = np.asarray(grid, dtype=np.float64)
    pts = grid.reshape(-1, 1) if grid.ndim == 1 else grid
    G = len(pts)
    lo, hi = (0.0, 1.0) if binary else (float(ranges[0]), float(ranges[1]))
    w, half = hi - lo, (0.0 if binary else 0.5)
    cancel = anchor is not None and not link
    cs, bs, sigs = [], [], []
    for p in parts:
        S = p["hit"].shape[0]
        nA = p["hit"].sum(axis=1)[None, :]
        lin, Z, ops = cc.linear(rows, S, offset, dense, p.get("dense_coef"), ell_index, ell_value, p.get("ell_coef"))
        ops = ops + (1 if offset is not None else 0)
        v, bv, order, Gs, sg = [], [], [], [], []
        for point in pts:
            xg = pc.overwritten(x, vars, point)
            bart = p["predict_bart"](xg).astype(LD)
            assert bart.shape == (rows, S)
            F, Ga, sig = leaf_walk(p["trees"], xg, p["hit"])
            o = (T + 2) * U * (F + half) * w + U * abs(lo)
            z = bart + lin
            A = (np.abs(bart) + Z).astype(np.float64)
            if link:
                pdf = sc.phi_pdf(z.astype(np.float64))
                v.append(sc.phi_cdf(z).astype(LD))
                bv.append(pdf * ((ops + 2) * U * A + o) + sc.ERFC_C * U)
            else:
                v.append(bart if cancel else z)
                bv.append(ops * U * A + o)
            order.append(o); Gs.append(Ga); sg.append(sig)
        v, bv, sg = np.stack(v, axis=1), np.stack(bv, axis=1), np.stack(sg, axis=1)          # [rows x G x S]
        if anchor is None:
            c, b = v, bv
        elif link:
            c = v - v[:, anchor:anchor + 1]
            b = bv + bv[:, anchor:anchor + 1] + U * np.abs(c).astype(np.float64)
        else:
            order, Gs = np.stack(order, axis=1), np.stack(Gs, axis=1)
            c = v - v[:, anchor:anchor + 1]
            GG = w * (Gs + Gs[:, anchor:anchor + 1])
            b = (nA[:, None, :] > 0) * (order + order[:, anchor:anchor + 1]) + (nA[:, None, :] + 2) * U * GG + 3.0 * U * GG
        if anchor is not None:
            same = sg == sg[:, anchor:anchor + 1]          # the anchor's exact-tie class: exactly 0 on both sides
            assert not c[same].any()
            b = np.where(same, 0.0, b)
        cs.append(c); bs.append(np.broadcast_to(b, c.shape)); sigs.append(sg)
    c, b, sig = np.concatenate(cs, axis=2), np.concatenate(bs, axis=2).astype(np.float64), np.concatenate(sigs, axis=2)
    S = c.shape[2]
    ref, bound = {"c": c}, {"c": b}
    sr, sb = sc.summarise(c.reshape(rows * G, S), b.reshape(rows * G, S))
    for key in ("mean", "m2"):
        ref[key], bound[key] = sr[key].reshape(rows, G), sb[key].reshape(rows, G)
    r = c.max(axis=1) - c.min(axis=1)
    br = 2.0 * b.max(axis=1) + U * np.abs(r).astype(np.float64)
    br = np.where((sig == sig[:, :1]).all(axis=1), 0.0, br)          # every grid point in one exact-tie class: max = min bit for bit, r is exactly 0
    ref["r"], bound["r"] = r, br
    rr, rb = sc.summarise(r, br)
    ref["range_mean"], ref["range_m2"], bound["range_mean"], bound["range_m2"] = rr["mean"], rr["m2"], rb["mean"], rb["m2"]
    if len(probs):
        Q = len(probs)
        ref["quantiles"] = qc.type7(c.reshape(rows * G, S), probs).astype(np.float64).reshape(Q, rows, G)
        bound["quantiles"] = qc.bound(c.reshape(rows * G, S).astype(np.float64), b.reshape(rows * G, S), Q).reshape(Q, rows, G)
        ref["range_quantiles"] = qc.type7(r, probs).astype(np.float64)
        bound["range_quantiles"] = qc.bound(r.astype(np.float64), br, Q)
    return ref, bound, {"sig": sig}


def counts(c, b, sig):
    """(certain_max, possible_max, certain_min, possible_min) [rows x G] as counts of draws, and the number of ambiguous (row, draw) pairs."""
    rows, G, S = c.shape
    out = [np.zeros((rows, G), dtype=np.int64) for _ in range(4)]
    ambiguous = 0
    lower = np.tril(np.ones((G, G), dtype=bool), -1)[:, :, None]          # [g, h]: h < g
    for i in range(rows):
        same = sig[i][:, None, :] == sig[i][None, :, :]                   # [g, h, k]
        diff = (c[i][:, None, :] - c[i][None, :, :]).astype(np.float64)   # c_g - c_h
        tol = b[i][:, None, :] + b[i][None, :, :]
        lowest = ~(same & lower).any(axis=1)                              # [g, k]
        cmax = lowest & (same | (diff > tol)).all(axis=1)
        pmax = lowest & ~(~same & (-diff > tol)).any(axis=1)
        cmin = lowest & (same | (-diff > tol)).all(axis=1)
        pmin = lowest & ~(~same & (diff > tol)).any(axis=1)
        for o, m in zip(out, (cmax, pmax, cmin, pmin)):
            o[i] = m.sum(axis=1)
        assert (cmax.sum(axis=0) <= 1).all() and (pmax.sum(axis=0) >= 1).all() and (cmin.sum(axis=0) <= 1).all() and (pmin.sum(axis=0) >= 1).all()
        ambiguous += int(((cmax.sum(axis=0) == 0) | (cmin.sum(axis=0) == 0)).sum())
    return (*out, ambiguous)


def lone_winners(ref, bound, extra):
    """[rows] bool: in every draw the row has a certain maximum and a certain minimum, each alone in its exact-tie class."""
    c, sig = ref["c"], extra["sig"]
    cmax, _, cmin, _, _ = counts(c, bound["c"], sig)
    S = c.shape[2]
    alone = np.ones(c.shape[0], dtype=bool)
    for pick in (c.argmax(axis=1), c.argmin(axis=1)):
        alone &= ((sig == np.take_along_axis(sig, pick[:, None, :], axis=1)).sum(axis=1) == 1).all(axis=1)
    return alone & (cmax.sum(axis=1) == S) & (cmin.sum(axis=1) == S)


def ambiguity(ref, bound, extra):
    rows, _, S = ref["c"].shape
    return counts(ref["c"], bound["c"], extra["sig"])[4] / float(rows * S)


def assert_curves(got, ref, bound, extra, what, report=print, keys=PER_POINT + ("range_mean", "range_m2", "range_quantiles")):
    """A Sampler.predict_curves result against model(): every entry of every output within BOUND_FACTOR x its bound, the shares inside their sandwich.
    The ratios are printed before they are asserted.  Returns the ratios."""
    ratios = {}
    for key in keys:
        if key in ref and got.get(key) is not None and np.size(got[key]):
            assert got[key].shape == ref[key].shape, (what, key, got[key].shape, ref[key].shape)
            ratios[key] = bound_ratio(got[key], ref[key], bound[key])
    S = ref["c"].shape[2]
    cmax, pmax, cmin, pmin, amb = counts(ref["c"], bound["c"], extra["sig"])
    info = got["info"]
    report(f"predict_curves {what}: route {info['route']}, {info['chunks']} chunk(s) of {info['rows_per_chunk']} rows, {S} draws, affected trees at most "
           f"{info['largest_affected']} / in all {info['total_affected']}, {amb} ambiguous (row, draw) pairs of {ref['c'].shape[0] * S}; "
           "max |device - model| / bound: " + ", ".join(f"{k} {r:.3g}" for k, r in ratios.items()))
    for key, r in ratios.items():
        assert r <= BOUND_FACTOR, f"{what}: {key} is {r:.3g} x the derived bound (allowed: {BOUND_FACTOR:g})"
    for key, lo, hi in (("p_max", cmax, pmax), ("p_min", cmin, pmin)):
        if got.get(key) is not None:
            n = np.rint(got[key] * S)          # the device divides an integer count by S: the same division gives the same bits back
            assert np.array_equal(n / float(S), got[key]) and np.array_equal(n.sum(axis=1), np.full(len(n), float(S))), (what, key, "not counts over S that add up to S")
            assert np.all(lo <= n) and np.all(n <= hi), f"{what}: {key} leaves its sandwich at {np.argwhere((lo > n) | (n > hi))[:5].tolist()}"
    return ratios


def brute_force(predict_bart, x, vars, grid, anchor=None):
    """Plain numpy, double precision, link 0, no linear part: the loop a user would write.  c [rows x G x S]."""
    grid = np.asarray(grid, dtype=np.float64)
    pts = grid.reshape(-1, 1) if grid.ndim == 1 else grid
    v = np.stack([predict_bart(pc.overwritten(x, vars, p)) for p in pts], axis=1)
    return v if anchor is None else v - v[:, anchor:anchor + 1]


# ---- chains and cases ------------------------------------------------------------------------------------------------------------------------------------
STEPS = (1, 1, 3, 8)          # stored samplers of 1, 2, 5 and 13 draws


def chain_args(kind):
    if kind == "gauss":
        return rc._friedman(n=300, T=20, warmup=4, iter=4 + sum(STEPS), ranef=False)
    if kind == "probit":
        return rc._binary(n=200, T=11, warmup=6, iter=6 + sum(STEPS))
    if kind == "unused":          # predictor 6 is constant in training: no tree splits on it
        args = rc._friedman(n=100, T=5, warmup=4, iter=4 + sum(STEPS), ranef=False)
        xb = np.array(args.x_bart, order="F")
        xb[:, 6] = 0.5
        args.x_bart = xb
        return args
    raise KeyError(kind)


def make_chain(lib, prefix, kind):
    return pc.Chain(lib, prefix, chain_args(kind), steps=STEPS, rows=300)


def busiest(chain, S, skip=()):
    """The predictor with the most affected trees in the stored sampler of S draws."""
    n = [(-1 if v in skip else chain.hit(S, v).sum()) for v in range(chain.P)]
    return int(np.argmax(n))


def grid_of(chain, vs, G, seed=0):
    """G points over the training range of the predictors widened by a fifth, in no order: [G] or [G x 2]."""
    g = np.random.default_rng(900 + seed)
    cols = []
    for v in vs:
        col = np.asarray(chain.args.x_bart)[:, v]
        lo, hi = col.min(), col.max()
        cols.append(g.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), G))
    return cols[0] if len(vs) == 1 else np.column_stack(cols)


# name -> dict(chain, pool (stored samplers by their draws, in pooling order), rows, G, V, anchor ("first", "last", None), link, M, E, offset,
# scratch_rows (rows per chunk the scratch is set for, or None), var ("busiest" or an index)).  Each GPU test runs its cases on both routes.
def _case(chain="gauss", pool=(2, 1), rows=65, G=5, V=1, anchor=None, link=0, M=0, E=0, offset=False, scratch_rows=None, var="busiest", seed=0):
    return dict(chain=chain, pool=pool, rows=rows, G=G, V=V, anchor=anchor, link=link, M=M, E=E, offset=offset, scratch_rows=scratch_rows, var=var, seed=seed)


CASES = {}
for _rows in (1, 63, 64, 65, 257):
    CASES[f"rows-{_rows}"] = _case(rows=_rows, anchor="first" if _rows % 2 else None, M=1, E=1)
CASES["chunks-4"] = _case(rows=200, scratch_rows=64, anchor="last", G=3)
CASES["chunks-4-plain"] = _case(rows=200, scratch_rows=64, G=3, link=0, M=1, offset=True)
for _G in (1, 2, 3, 4, 5, 64):
    CASES.setdefault(f"grid-{_G}-anchor", _case(rows=70, G=_G, anchor="last", seed=_G))
    CASES.setdefault(f"grid-{_G}", _case(rows=70, G=_G, seed=_G, E=1))
for _S, _pool in ((1, (1,)), (7, (5, 2)), (8, (5, 2, 1)), (9, (5, 2, 1, 1)), (16, (13, 2, 1)), (17, (13, 2, 1, 1)), (70, (13,) * 5 + (5,))):
    CASES[f"draws-{_S}"] = _case(pool=_pool, rows=40 if _S > 20 else 80, G=5, anchor="first" if _S % 2 else None, M=1, seed=_S)
CASES["pair"] = _case(V=2, G=9, rows=100, pool=(5, 1))
CASES["pair-anchor"] = _case(V=2, G=9, rows=100, pool=(5, 1), anchor="first")
CASES["probit"] = _case(chain="probit", link=1, rows=130, G=6, pool=(5, 2), M=1, E=2, offset=True)
CASES["probit-anchor-first"] = _case(chain="probit", link=1, rows=130, G=6, pool=(5, 2), anchor="first", M=1)
CASES["probit-anchor-last"] = _case(chain="probit", link=1, rows=70, G=3, pool=(2, 1), anchor="last", E=1)
CASES["probit-latent-anchor"] = _case(chain="probit", link=0, rows=70, G=5, pool=(5,), anchor="first")
CASES["parts"] = _case(rows=90, G=4, pool=(5, 2), M=2, E=3, offset=True)
CASES["parts-anchor"] = _case(rows=90, G=4, pool=(5, 2), M=2, E=3, offset=True, anchor="last")


def inputs(chain, case):
    """What a case hands to Sampler.predict_curves and to model(): dict(x, vars, grid, anchor, link, pool, call: keyword arguments of the call on the
    first pooled sampler, parts: model()'s, linear: model()'s row side)."""
    S0, rows, G = case["pool"][0], case["rows"], case["G"]
    first = busiest(chain, 13) if case["var"] == "busiest" else int(case["var"])
    vs = [first] if case["V"] == 1 else [first, busiest(chain, 13, skip=(first,))]
    grid = grid_of(chain, vs, G, seed=case["seed"])
    anchor = {None: None, "first": 0, "last": G - 1}[case["anchor"]]
    x = np.asfortranarray(chain.x[:rows])
    tables = [sc.linear_parts(rows, S, case["M"], case["E"], seed=case["seed"] + 31 * j) for j, S in enumerate(case["pool"])]
    side = sc.linear_parts(rows, S0, case["M"], case["E"], seed=case["seed"])          # the row side is the first sampler's
    # (under link 1 a large offset saturates Phi: many grid points at exactly 0 or 1, ties outside every class)
    scale = 0.5 if case["link"] else 10.0 * float(chain.range[1] - chain.range[0])
    off = scale * np.random.default_rng(case["seed"]).uniform(-1.0, 1.0, rows) if case["offset"] else None
    linear = dict(offset=off, dense=side.get("dense"), ell_index=side.get("ell_index"), ell_value=side.get("ell_value"))
    Stot = sum(case["pool"])
    call = dict(linear, dense_coef=tables[0].get("dense_coef"), ell_coef=tables[0].get("ell_coef"), link=case["link"], anchor=anchor,
                peer_dense_coef=[t["dense_coef"] for t in tables[1:]] if case["M"] and len(tables) > 1 else None,
                peer_ell_coef=[t["ell_coef"] for t in tables[1:]] if case["E"] and len(tables) > 1 else None,
                scratch_bytes=8 * case["scratch_rows"] * Stot * G if case["scratch_rows"] else 0)
    parts = [dict(predict_bart=chain.stored[S].predict_bart, trees=chain.trees[S], hit=chain.hit(S, vs), dense_coef=t.get("dense_coef"), ell_coef=t.get("ell_coef"))
             for S, t in zip(case["pool"], tables)]
    return dict(x=x, vars=vs, grid=grid, anchor=anchor, link=case["link"], pool=case["pool"], call=call, parts=parts, linear=linear)


def case_model(chain, inp, probs=PROBS):
    return model(inp["parts"], inp["x"], inp["vars"], inp["grid"], chain.T, chain.range, chain.binary, anchor=inp["anchor"], link=inp["link"], probs=probs,
                 **inp["linear"])
