"""s4b_partial_dependence (stan4bart_amd/csrc/dev_pd.inc over dev_readout.inc: k_partial_dependence<staged / global>, k_summary_fold) — the model, the bound, the tree-order
restatement and the chains shared by tests/test_partial_dependence.py (CPU) and tests/test_gpu_partial_dependence.py (GPU).

The reference.  For every grid point g the rows get their column(s) `vars` overwritten by the grid point's value(s) and go through predict_bart of the
same sampler (k_predict, held to the numpy walk by tests/test_gpu_readout.py); the [rows x draws] matrix then goes through summary_cases.model: the
linear parts (at the rows' own values) in np.longdouble, the link, the weighted row sum.

The bound of pd[k, g] is summary_cases' bound of `average` — but there the BART term enters as an exact term, because k_predict_summary adds the trees
in k_predict's order.  k_partial_dependence adds the trees without a rule on a varied predictor first and the others afterwards: the same T terms in
another order, so its BART term and predict_bart's each carry the rounding of a T-term sum.  Per (row, draw, grid point) the bound of v is therefore
widened by readout_cases' derived term of such a sum,
    (T + 2) u (sum_t |mu_t| + 0.5) (max - min) + u |min|          (binary response: range 1, min 0, no + 0.5: there is no rescale),
with sum_t |mu_t| from readout_cases.walk_leaves over get_kept_trees() at the overwritten rows; under link 1 it is carried through Phi' = phi(z).  It
enters pd's bound weighted by |w|, as every error of v does.  The tests allow readout_cases.BOUND_FACTOR x the bound."""
import numpy as np

import readout_cases as rc
import summary_cases as sc
from readout_cases import BOUND_FACTOR, U  # noqa: F401


# ---- the tree order of a call, restated ----------------------------------------------------------------------------------------------------------------
def affected(trees, vars, S, T):
    """[S x T] bool from a flattened tree list (get_kept_trees()): does tree t of draw k hold a rule on one of `vars`?"""
    hit = np.zeros((S, T), dtype=bool)
    on = np.isin(trees["var"], np.atleast_1d(vars)) & (trees["var"] >= 0)
    sample = trees["sample"] if "sample" in trees else np.zeros(len(trees["var"]), dtype=np.int64)
    hit[sample[on], trees["tree"][on]] = True
    return hit


def tree_order(hit):
    """SamplerCore::pd_tree_order restated: per draw the trees without such a rule in ascending index, then the others in ascending index, and the size
    of the first group."""
    order = np.array([np.r_[np.flatnonzero(~h), np.flatnonzero(h)] for h in hit], dtype=np.int32).reshape(hit.shape)
    return order, (~hit).sum(axis=1).astype(np.int32)


def make_trees(draws):
    """A flattened tree list in get_kept_trees()' layout from handwritten trees: draws[k][t] is a preorder list of entries, (var, cut value) for a rule
    and a float for a leaf."""
    var, value, tree, sample = [], [], [], []
    for k, trees in enumerate(draws):
        for t, entries in enumerate(trees):
            for e in entries:
                rule = isinstance(e, tuple)
                var.append(e[0] if rule else -1)
                value.append(float(e[1] if rule else e))
                tree.append(t)
                sample.append(k)
    return dict(var=np.array(var, dtype=np.int32), value=np.array(value), tree=np.array(tree, dtype=np.int32), sample=np.array(sample, dtype=np.int32))


# ---- the reference and its bound -----------------------------------------------------------------------------------------------------------------------
def overwritten(x, vars, point):
    xg = np.array(x, dtype=np.float64, order="F")
    for v, c in zip(np.atleast_1d(vars), np.atleast_1d(point)):
        xg[:, v] = c
    return xg


def reference(predict_bart, trees, ranges, binary, x, vars, grid, weights=None, link=0, offset=None, **parts):
    """(pd [S x G], bound [S x G]).  `predict_bart`: rows -> [rows x S]; `trees`: get_kept_trees() of the same draws; `ranges`: (min, max) of the response
    scale, one pair or one per draw; `grid` [G] or [G x len(vars)]; `weights` None (1 / rows) or [rows]; `parts`: dense, dense_coef, ell_*."""
    x = np.asarray(x, dtype=np.float64)
    rows = x.shape[0]
    grid = np.asarray(grid, dtype=np.float64)
    pts = grid.reshape(-1, 1) if grid.ndim == 1 else grid
    w = np.full(rows, 1.0 / rows) if weights is None else np.asarray(weights, dtype=np.float64)
    starts, _ = rc.tree_starts(trees)
    draw = trees["sample"][starts].astype(np.int64)
    S = int(draw.max()) + 1
    T = len(starts) // S
    ranges = np.broadcast_to(np.asarray(ranges, dtype=np.float64).reshape(-1, 2), (S, 2))
    lo, width = ranges[:, 0], ranges[:, 1] - ranges[:, 0]
    pd, bound = np.zeros((S, len(pts))), np.zeros((S, len(pts)))
    for g, point in enumerate(pts):
        xg = overwritten(x, vars, point)
        bart = predict_bart(xg)
        assert bart.shape == (rows, S)
        fabs = np.zeros((rows, S))
        for a, _, pos in rc.walk_leaves(trees, xg):
            fabs[:, draw[a]] += np.abs(trees["value"][pos])
        order_term = (T + 2) * U * fabs if binary else (T + 2) * U * (fabs + 0.5) * width[None, :] + U * np.abs(lo)[None, :]
        ref, b = sc.model(bart, offset, link=link, weights=w[None, :], **parts)
        if link:
            z, _ = sc.model(bart, offset, link=0, **parts)
            order_term = sc.phi_pdf(z["v"]) * order_term
        pd[:, g] = ref["average"][:, 0]
        bound[:, g] = b["average"][:, 0] + np.abs(w) @ order_term
    return pd, bound


def assert_pd(got, ref, bound, what, report=print):
    """A Sampler.partial_dependence result against reference(): every entry within BOUND_FACTOR x its bound; the largest ratio is printed first."""
    assert got["pd"].shape == ref.shape, (what, got["pd"].shape, ref.shape)
    r = rc.bound_ratio(got["pd"], ref, bound)
    info = got["info"]
    report(f"partial_dependence {what}: route {info['route']}, {info['workgroups']} workgroup(s), affected trees at most {info['largest_affected']} / in all "
           f"{info['total_affected']}; max |device - model| / bound = {r:.3g}")
    assert r <= BOUND_FACTOR, f"{what}: pd is {r:.3g} x the derived bound (allowed: {BOUND_FACTOR:g})"
    return r


def brute_force(predict_bart, x, vars, grid, weights=None):
    """Plain numpy, double precision: the loop a user would write (link 0, no linear part)."""
    grid = np.asarray(grid, dtype=np.float64)
    pts = grid.reshape(-1, 1) if grid.ndim == 1 else grid
    w = np.full(len(x), 1.0 / len(x)) if weights is None else np.asarray(weights, dtype=np.float64)
    return np.column_stack([w @ predict_bart(overwritten(x, vars, p)) for p in pts])


# ---- chains --------------------------------------------------------------------------------------------------------------------------------------------
class Chain:
    """One chain: the live sampler and stored samplers holding its first sum(steps[:j]) draws, each with its kept trees; new rows to average over."""

    def __init__(self, lib, prefix, args, steps=(1, 1, 3, 8), rows=2200, seed=3):
        from conftest import make_sampler
        from stan4bart_amd.abi import StoredSampler
        assert args.keep_trees and args.iter - args.warmup == sum(steps)
        self.args, self.live, self.stored, self.trees, kept = args, make_sampler(lib, prefix, args), {}, {}, 0
        try:
            if args.warmup:
                self.live.run(args.warmup, True)
            self.live.disengage_adaptation()
            for more in steps:
                self.live.run(more, False)
                kept += more
                self.stored[kept] = StoredSampler(lib, prefix, self.live.export_bart_state())
                self.trees[kept] = self.stored[kept].get_kept_trees()
            self.draws, self.T, self.P = kept, args.n_trees, args.x_bart.shape[1]
            self.binary = bool(args.is_binary)
            self.range = self.live.get_bart_data_range()
            self.x = rc.new_rows(args.x_bart, rows, seed=seed)
        except Exception:
            self.close()
            raise

    def hit(self, S, vars):
        return affected(self.trees[S], vars, S, self.T)

    def reference(self, S, rows, vars, grid, **kw):
        return reference(self.stored[S].predict_bart, self.trees[S], self.range, self.binary, self.x[:rows], vars, grid, **kw)

    def close(self):
        for st in self.stored.values():
            st.free()
        self.live.free()
