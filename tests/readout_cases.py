"""The kernels that read results OUT of the trees — k_predict (predict() of the kept draws), k_test_fits_few / k_test_fits (per-iteration fits of the
test rows), k_var_counts, k_draw_k (stan4bart_amd/csrc/dev_hip.hip) — at the shapes that select their branches: the reference, the branch functions and
the case builders shared by tests/test_gpu_readout.py (GPU) and its CPU twin tests/test_readout.py (the same builders over the emulated device layer).

The reference (walk_fits) is a vectorised numpy walk of the FLATTENED trees as get_trees() / get_kept_trees() return them (preorder; `value` is the raw
cut value at a rule, the leaf value on the internal scale at a leaf) over the RAW test matrix.  It never sees bin indices, PackedNode, node links or
SamplerCore::bin_matrix: agreement with it checks binning, packing, links, the walk, the summation and the response scale at once.

Tolerance (written once, here: walk_fits returns it).  The device adds the T leaf values of a row in double precision in the order of the trees (T - 1 roundings of
partial sums no larger than sum |mu_t|), adds 0.5 (one rounding), multiplies by the range and adds the minimum (two roundings, or one if contracted
to a multiply-add): the error of f + 0.5 is at most T * u * (sum |mu_t| + 0.5) with u = 2^-53, the product carries it times (max - min) plus one more
relative rounding, the final sum rounds once more relative to a result no larger than (sum |mu_t| + 0.5) * (max - min) + |min|.  Together at most
    (T + 2) * u * (sum |mu_t| + 0.5) * (max - min) + u * |min|
per entry; for a binary response (no scale: the sum itself) (T + 2) * u * sum |mu_t|.  The tests assert |device - reference| <= 4 x this bound, computed
per entry from the reference's own sum of |mu_t| (the factor 4: the long-double reference's own roundings — 80-bit where the platform has it, plain
double where it has not — and the final conversion to double)."""
import copy
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
BOUND_FACTOR = 4.0


# ---- which kernel / branch a shape selects --------------------------------------------------------------------------------------------------------------
def readout_limits():
    """The constants that shape the read-out launches, READ from dev_hip.hip (and the host's binning threshold from sampler_core.hpp); the statements
    the branch functions below restate are asserted to still be there, so that a moved threshold or a reshaped launch fails here."""
    src = open(os.path.join(ROOT, "stan4bart_amd", "csrc", "dev_hip.hip")).read()
    core = open(os.path.join(ROOT, "stan4bart_amd", "csrc", "sampler_core.hpp")).read()

    def const(name):
        return int(re.search(r"constexpr int " + name + r" = (\d+);", src).group(1))
    lim = dict(block=const("BLOCK"), grid_max=const("GRID_MAX"))
    assert "constexpr int TF_ROWS = BLOCK / 64;" in src
    lim["tf_rows"] = lim["block"] // 64
    assert "const size_t lds = (size_t)TF_ROWS * (size_t)T_ * 8;" in src
    m = re.search(r"if \(nTest_ <= (\d+) && lds <= (\d+) \* 1024\)", src)
    lim["few_rows"], lim["few_lds"] = int(m.group(1)), int(m.group(2)) * 1024
    assert "std::min<int64_t>(GRID_MAX, std::max<int64_t>(1, (nTest_ + TF_ROWS - 1) / TF_ROWS))" in src
    assert "std::min<int64_t>(GRID_MAX, std::max<int64_t>(1, (nTest_ + BLOCK - 1) / BLOCK))" in src
    assert "for (int t = lane; t < a.T; t += 64)" in src
    m = re.search(r"std::min<int64_t>\((\d+), std::max<int64_t>\(1, \(total \+ BLOCK - 1\) / BLOCK\)\);\s*hipLaunchKernelGGL\(k_predict,", src)
    lim["predict_grid"] = int(m.group(1))
    assert "hipLaunchKernelGGL(k_var_counts, dim3(1), dim3(BLOCK)" in src
    assert "for (int j = threadIdx.x; j < a.P; j += BLOCK) out[j] = 0;" in src and "for (int t = threadIdx.x; t < a.T; t += BLOCK) {" in src
    assert "hipLaunchKernelGGL(k_draw_k, dim3(1), dim3(256)" in src and "for (int t = threadIdx.x; t < a.T; t += 256)" in src
    lim["draw_k_block"] = 256
    m = re.search(r"if \(\(size_t\)P_ \* m < \(1u << (\d+)\)\) nt = 1;", core)
    lim["bin_threads_from"] = 1 << int(m.group(1))
    return lim


def _ceil(a, b):
    return -(-a // b)


def fits_branch(n_test, T):
    """kernel ("few": k_test_fits_few, a thread per (row, tree); "rows": k_test_fits, a thread per row), workgroups, how often the kernel's outer loop
    goes round, rows that sit idle in its last round (few only), trees a lane walks (few only)."""
    L = readout_limits()
    if n_test <= L["few_rows"] and L["tf_rows"] * T * 8 <= L["few_lds"]:
        grid = min(L["grid_max"], max(1, _ceil(n_test, L["tf_rows"])))
        per_round = grid * L["tf_rows"]
        return dict(kernel="few", grid=grid, rounds=_ceil(n_test, per_round), idle_rows=_ceil(n_test, L["tf_rows"]) * L["tf_rows"] - n_test,
                    trees_per_lane=_ceil(T, 64), lds=L["tf_rows"] * T * 8)
    grid = min(L["grid_max"], max(1, _ceil(n_test, L["block"])))
    return dict(kernel="rows", grid=grid, rounds=_ceil(n_test, grid * L["block"]), idle_rows=0, trees_per_lane=T, lds=0)


def predict_branch(rows, draws, P):
    """k_predict: workgroups, rounds of its grid-stride loop, elements per round, and whether the host bins the new rows on a thread pool."""
    L = readout_limits()
    total = rows * draws
    grid = min(L["predict_grid"], max(1, _ceil(total, L["block"])))
    return dict(grid=grid, per_round=grid * L["block"], rounds=_ceil(total, grid * L["block"]), threaded_binning=P * rows >= L["bin_threads_from"])


def counts_branch(P, T):
    """k_var_counts / k_draw_k: rounds of the clearing loop over predictors, of the loops over trees."""
    L = readout_limits()
    return dict(p_rounds=_ceil(P, L["block"]), t_rounds=_ceil(T, L["block"]), k_rounds=_ceil(T, L["draw_k_block"]))


# ---- the reference: a vectorised walk of the flattened trees -------------------------------------------------------------------------------------------
def _subtree_ends(var):
    """For every entry of a preorder node list the index one past its subtree (one backward pass)."""
    m = len(var)
    end = np.empty(m, dtype=np.int64)
    for i in range(m - 1, -1, -1):
        end[i] = i + 1 if var[i] < 0 else end[end[i + 1]]          # a rule: left subtree at i + 1, right subtree where the left one ends
    return end


def tree_starts(trees):
    """First entry of every tree of a flattened tree list, found from the preorder structure alone; checked against the (sample, tree) labels."""
    var = trees["var"]
    end = _subtree_ends(var)
    starts, i = [], 0
    while i < len(var):
        starts.append(i)
        i = int(end[i])
    starts = np.asarray(starts, dtype=np.int64)
    label = trees["tree"].astype(np.int64) + (trees["sample"].astype(np.int64) << 32 if "sample" in trees else 0)
    assert np.array_equal(starts, np.flatnonzero(np.r_[True, np.diff(label) != 0])), "the (sample, tree) labels do not follow the preorder structure"
    return starts, end


def walk_leaves(trees, x):
    """The walk alone: for every tree of a flattened tree list, in order, the ENTRY index of the leaf that each raw row of `x` reaches ("go left iff
    x <= cut value").  Yields (position of the tree in the list, its first entry, entry index per row).  walk_fits sums the leaf values found this
    way; tests/handoff_cases.py (audit_state) compares the leaves themselves with the device's leaf assignment."""
    x = np.asarray(x, dtype=np.float64)
    var, value = trees["var"], trees["value"]
    starts, end = tree_starts(trees)
    m = x.shape[0]
    rows = np.arange(m)
    for a, st in enumerate(starts):
        pos = np.full(m, st, dtype=np.int64)
        act = rows if var[st] >= 0 else rows[:0]
        while len(act):
            p = pos[act]
            left = x[act, var[p]] <= value[p]
            p = np.where(left, p + 1, end[p + 1])
            pos[act] = p
            act = act[var[p] >= 0]
        yield a, int(st), pos


def walk_fits(trees, x, ranges, binary=False):
    """Fits [rows x draws] of the raw rows `x` under the flattened `trees` (get_kept_trees(): every kept draw; get_trees(): one draw), `ranges` the
    (min, max) of the response scale of every draw ([draws x 2], or one pair for all).  Returns (fits as float64, the bound of the module docstring per
    entry, sum |mu_t| per entry is folded into it)."""
    x = np.asarray(x, dtype=np.float64)
    var, value = trees["var"], trees["value"]
    starts, end = tree_starts(trees)
    draw = trees["sample"][starts].astype(np.int64) if "sample" in trees else np.zeros(len(starts), dtype=np.int64)
    S = int(draw.max()) + 1
    T = len(starts) // S
    assert len(starts) == S * T and np.array_equal(draw, np.repeat(np.arange(S), T)) and np.array_equal(trees["tree"][starts], np.tile(np.arange(T), S))
    ranges = np.broadcast_to(np.asarray(ranges, dtype=np.float64).reshape(-1, 2), (S, 2))
    m = x.shape[0]
    f = np.zeros((m, S), dtype=np.longdouble)
    fabs = np.zeros((m, S), dtype=np.longdouble)
    for a, st, pos in walk_leaves(trees, x):
        mu = value[pos].astype(np.longdouble)
        f[:, draw[a]] += mu
        fabs[:, draw[a]] += np.abs(mu)
    lo, hi = ranges[:, 0].astype(np.longdouble), ranges[:, 1].astype(np.longdouble)
    if binary:
        return f.astype(np.float64), ((T + 2) * U * fabs).astype(np.float64)
    out = (f + np.longdouble(0.5)) * (hi - lo)[None, :] + lo[None, :]
    bound = (T + 2) * U * (fabs + np.longdouble(0.5)) * (hi - lo)[None, :] + U * np.abs(lo)[None, :]
    return out.astype(np.float64), bound.astype(np.float64)


def bound_ratio(device, reference, bound):
    """Largest |device - reference| / bound (0 / 0 counts as 0: a single tree's leaf value of a binary response is exact on both sides)."""
    d = np.abs(np.asarray(device, dtype=np.longdouble) - np.asarray(reference, dtype=np.longdouble)).astype(np.float64)
    assert np.all(np.isfinite(d)), "a device result or the reference is not finite"
    r = np.divide(d, bound, out=np.zeros_like(d), where=d > 0)
    return float(r.max()) if r.size else 0.0


def assert_within_bound(device, reference, bound, what):
    r = bound_ratio(device, reference, bound)
    assert r <= BOUND_FACTOR, f"{what}: |device - reference| is {r:.3g} x the derived bound (allowed: {BOUND_FACTOR:g})"
    return r


def nodes_per_tree(trees):
    starts, _ = tree_starts(trees)
    return np.diff(np.r_[starts, len(trees["var"])])


def count_rules(trees, P, draws=None):
    """varcount from the flattened trees: entries with var >= 0 per predictor [P] (get_trees()) or per predictor and draw [P x draws] (get_kept_trees())."""
    rule = trees["var"] >= 0
    if "sample" not in trees:
        return np.bincount(trees["var"][rule], minlength=P).astype(np.int32)
    out = np.zeros((P, draws), dtype=np.int32)
    np.add.at(out, (trees["var"][rule], trees["sample"][rule]), 1)
    return out


# ---- rows built to be hard -----------------------------------------------------------------------------------------------------------------------------
def rule_list(trees, max_deeper=200, seed=0):
    """(root rules, deeper rules) of a flattened tree list as arrays of (predictor, raw cut value): every root rule, and up to `max_deeper` of the others
    from every depth (a seeded choice)."""
    starts, _ = tree_starts(trees)
    var, value = trees["var"], trees["value"]
    roots = starts[var[starts] >= 0]
    other = np.setdiff1d(np.flatnonzero(var >= 0), roots)
    if len(other) > max_deeper:
        other = np.sort(np.random.default_rng(seed).choice(other, max_deeper, replace=False))
    return (var[roots].astype(np.int64), value[roots].copy()), (var[other].astype(np.int64), value[other].copy())


def hard_rows(x_train, roots, deeper, seed=0):
    """Rows at the places where binning and walk have to agree with "go left iff x <= cut value".  For every rule three rows that differ in the rule's
    predictor only — exactly the cut value (left), nextafter(cut, +inf) (right), nextafter(cut, -inf) (left) — the other columns a seeded training row;
    then rows at +-inf, +-1e300 and ten times the training range outside it in every column, the column minima and maxima.
    Returns (rows, n_root): rows [3 * r : 3 * r + 3] belong to root rule r for r < n_root, the deeper rules follow in the same layout."""
    g = np.random.default_rng(1000 + seed)
    x_train = np.asarray(x_train, dtype=np.float64)
    n, P = x_train.shape
    v = np.concatenate([roots[0], deeper[0]])
    c = np.concatenate([roots[1], deeper[1]])
    base = x_train[g.integers(0, n, len(v))].copy()
    trip = np.repeat(base, 3, axis=0)
    k = np.arange(len(v))
    trip[3 * k, v] = c
    trip[3 * k + 1, v] = np.nextafter(c, np.inf)
    trip[3 * k + 2, v] = np.nextafter(c, -np.inf)
    lo, hi = x_train.min(axis=0), x_train.max(axis=0)
    far = 10.0 * (hi - lo) + 1.0
    edge = np.vstack([np.full(P, np.inf), np.full(P, -np.inf), np.full(P, 1e300), np.full(P, -1e300), hi + far, lo - far, lo, hi,
                      np.where(np.arange(P) % 2 == 0, np.inf, -np.inf), np.where(np.arange(P) % 2 == 0, -1e300, 1e300)])
    return np.vstack([trip, edge]), len(roots[0])


def new_rows(x_train, m, seed=0):
    """m rows that are not training rows: uniform draws over the training range of every column widened by a tenth on both sides."""
    g = np.random.default_rng(2000 + seed)
    x_train = np.asarray(x_train, dtype=np.float64)
    lo, hi = x_train.min(axis=0), x_train.max(axis=0)
    w = hi - lo
    out = np.empty((m, x_train.shape[1]), order="F")
    for j in range(x_train.shape[1]):
        out[:, j] = g.uniform(lo[j] - 0.1 * w[j], hi[j] + 0.1 * w[j], m)
    return out


def assert_root_rule_rows(fits, n_root, draw):
    """For rows built from ROOT rules (every row meets them): the fit of `draw` must differ between `cut` and nextafter(cut, +inf) for at least half of
    them, and `cut` and nextafter(cut, -inf) must give equal fits in EVERY draw.  Returns how many differed."""
    k = np.arange(n_root)
    at, above, below = fits[3 * k], fits[3 * k + 1], fits[3 * k + 2]
    assert np.array_equal(at, below), "a value just below a root cut and the cut value itself gave different fits"
    differed = int(np.sum(at[:, draw] != above[:, draw]))
    assert 2 * differed >= n_root, f"only {differed} of {n_root} root-rule rows change between the cut value and the next double above it"
    return differed


# ---- chains ---------------------------------------------------------------------------------------------------------------------------------------------
def run_readout(lib, prefix, args, seed=12345, then=None, trace=True):
    """conftest.run_chain restricted to what assert_chain_parity compares, plus: the kept trees, and `then(sampler, out)` called before the sampler is freed
    (predictions, exported states)."""
    from conftest import make_sampler
    s = make_sampler(lib, prefix, args, seed)
    out = {}
    try:
        if trace:
            s.set_trace(True)
        traces = []
        if args.warmup > 0:
            out["warmup"] = s.run(args.warmup, True, 0)
            if trace:
                traces.append(s.get_trace())
        s.disengage_adaptation()
        out["sample"] = s.run(args.iter - args.warmup, False, 0)
        if trace:
            traces.append(s.get_trace())
            out["trace"] = np.concatenate(traces)
        out["trees"] = s.get_trees()
        if args.keep_trees:
            out["kept_trees"] = s.get_kept_trees()
        out["rng"] = s.get_r_rng_state()
        out["leaf0"] = s.get_leaf_assignment(0)
        out["range"] = s.get_bart_data_range()
        if then is not None:
            then(s, out)
    finally:
        s.free()
    return out


def with_test_rows(args, x_test):
    a = copy.copy(args)
    a.x_test = np.asfortranarray(x_test)
    return a


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------------------
def _friedman(**kw):
    from conftest import friedman_case
    keep = kw.pop("keep_trees", True)
    args, _ = friedman_case(**kw)
    args.keep_trees = keep
    return args


def _sized(n, **kw):
    from large_cases import sized_case
    keep = kw.pop("keep_trees", True)
    args = sized_case(n, **kw)
    args.keep_trees = keep
    return args


def _binary(**kw):
    from conftest import binary_case
    keep = kw.pop("keep_trees", True)
    args = binary_case(**kw)
    args.keep_trees = keep
    return args


def _quantile_case():
    """Quantile cuts with a different number of cuts per predictor: predictor 0 with n.cuts = 1000 (cut indices beyond 255), 1 with n.cuts = 0 (no rule
    can use it), 2 rounded to 11 distinct values (10 cuts although 100 were asked for), 3 binary (1 cut), the others 7 ... 100."""
    args = _friedman(n=2000, T=20, warmup=6, iter=12, ranef=False)
    xb = np.array(args.x_bart, order="F")
    xb[:, 2] = np.round(xb[:, 2], 1)
    xb[:, 3] = (xb[:, 3] > 0.5).astype(np.float64)
    args.x_bart = xb
    args.n_cuts = [1000, 0, 100, 100, 7, 100, 33, 64, 100]
    args.use_quantiles = True
    return args


def _c5_case():
    args = _friedman(n=1500, p=141, T=200, warmup=3, iter=7, ranef=False)
    assert args.x_bart.shape[1] == 140
    return args


# name -> (builder of the sampler arguments, rows of predict_bart's new matrix, kept draws).  n stays small wherever the branch is chosen by rows x draws
# alone: predict_bart costs no oracle time (the reference is the numpy walk), its cost is the chain on the device and the walk on the host.
PREDICT_CASES = {
    # rows x draws against the 4096 workgroups x 256 threads of k_predict: exactly one round; one element into the second; four rounds, the last of 36
    "cap-exact": (lambda: _friedman(n=400, T=5, warmup=4, iter=12, ranef=False), 131072, 8),
    "cap-plus-1": (lambda: _friedman(n=400, T=5, warmup=4, iter=21, ranef=False), 61681, 17),
    "three-caps": (lambda: _friedman(n=400, T=4, warmup=4, iter=16, ranef=False), 262147, 12),
    "one-row": (lambda: _friedman(n=400, T=12, warmup=4, iter=16, ranef=False), 1, 12),
    "one-draw": (lambda: _friedman(n=400, T=12, warmup=6, iter=7, ranef=False), 5000, 1),
    # P * rows >= 2^22: SamplerCore::bin_matrix bins the new rows on a thread pool
    "threaded-binning": (lambda: _friedman(n=400, T=4, warmup=4, iter=6, ranef=False), 500000, 2),
    # BASELINE config 5's shape at reduced n: 200 trees, 140 predictors
    "c5-200x140": (_c5_case, 2000, 4),
    # trees of more than 128 nodes (deep prior, 1024 node slots): links into slots beyond the first 128
    "deep": (lambda: _sized(3000, seed=1, p=10, trees=20, iters=(2, 6), deep=True), 2000, 4),
    "quantile-cuts": (_quantile_case, 2000, 6),
    "binary": (lambda: _binary(n=400, T=11, warmup=6, iter=12), 2000, 6),
    "hard-rows": (lambda: _friedman(n=2000, T=25, warmup=6, iter=10, ranef=False), 0, 4),
}

# name -> (builder without test rows, n_test, T).  The test rows are the hard rows of the chain's own rules (found by a first run of the same chain
# without test rows: they do not enter the chain) filled up with new_rows.  n stays small: the branch is chosen by n_test and T alone, and the oracle
# walks every test row through every tree on one thread.
TEST_FIT_CASES = {}
for _m in (1, 3, 4, 5, 8192, 8193, 65536, 65537):
    TEST_FIT_CASES["rows-%d" % _m] = (lambda: _friedman(n=400, T=9, warmup=3, iter=6, ranef=False), _m, 9)
TEST_FIT_CASES["rows-524800"] = (lambda: _friedman(n=400, T=3, warmup=2, iter=4, ranef=False, keep_trees=False), 524800, 3)
for _t in (64, 65, 130, 300):
    TEST_FIT_CASES["trees-%d" % _t] = ((lambda t: lambda: _friedman(n=400, T=t, warmup=2, iter=5, ranef=False))(_t), 300, _t)
for _t in (1536, 1537):
    TEST_FIT_CASES["trees-%d" % _t] = ((lambda t: lambda: _friedman(n=300, T=t, warmup=1, iter=3, ranef=False))(_t), 11, _t)
TEST_FIT_CASES["probit-few"] = (lambda: _binary(n=300, T=11, warmup=3, iter=6), 401, 11)
TEST_FIT_CASES["probit-rows"] = (lambda: _binary(n=300, T=5, warmup=2, iter=4), 65600, 5)

# what every case is FOR: (kernel, rounds of its outer loop, idle rows in the last round > 0, trees per lane) — fits_branch must say the same
TEST_FIT_EXPECTED = {
    "rows-1": ("few", 1, True, 1), "rows-3": ("few", 1, True, 1), "rows-4": ("few", 1, False, 1), "rows-5": ("few", 1, True, 1),
    "rows-8192": ("few", 1, False, 1), "rows-8193": ("few", 2, True, 1), "rows-65536": ("few", 8, False, 1), "rows-65537": ("rows", 1, False, 9),
    "rows-524800": ("rows", 2, False, 3), "trees-64": ("few", 1, False, 1), "trees-65": ("few", 1, False, 2), "trees-130": ("few", 1, False, 3),
    "trees-300": ("few", 1, False, 5), "trees-1536": ("few", 1, True, 24), "trees-1537": ("rows", 1, False, 1537),
    "probit-few": ("few", 1, True, 1), "probit-rows": ("rows", 1, False, 5),
}
# (rounds of k_predict's grid-stride loop, threaded binning)
PREDICT_EXPECTED = {
    "cap-exact": (1, False), "cap-plus-1": (2, False), "three-caps": (4, False), "one-row": (1, False), "one-draw": (1, False),
    "threaded-binning": (1, True), "c5-200x140": (1, False), "deep": (1, False), "quantile-cuts": (1, False), "binary": (1, False), "hard-rows": (1, False),
}

COUNT_CASES = {
    # T = 300: the tree loops of k_var_counts (t += 256) and, with a chi hyperprior on k, of k_draw_k go round twice
    "trees-300": (lambda: _friedman(n=600, T=300, warmup=3, iter=7, ranef=False, n_test=37), 9, 300),
    "trees-300-chi-k": (lambda: _friedman(n=600, T=300, warmup=3, iter=7, ranef=False, n_test=37, bart_args={"k": ("chi", 1.25, float("inf"))}), 9, 300),
    # 299 predictors: the clearing loop of k_var_counts goes round twice; rules on predictors >= 256 must have been accepted
    "predictors-299": (lambda: _friedman(n=900, p=300, T=12, warmup=4, iter=12, ranef=False, n_test=37), 299, 12),
}
COUNT_EXPECTED = {"trees-300": (1, 2), "trees-300-chi-k": (1, 2), "predictors-299": (2, 1)}          # (p_rounds, t_rounds)


def check_predict_branch(name, args, rows):
    draws = args.iter - args.warmup
    br = predict_branch(rows, draws, args.x_bart.shape[1])
    assert (br["rounds"], br["threaded_binning"]) == PREDICT_EXPECTED[name], (name, br)
    return br


def check_test_fit_branch(name, n_test, T):
    br = fits_branch(n_test, T)
    assert (br["kernel"], br["rounds"], br["idle_rows"] > 0, br["trees_per_lane"]) == TEST_FIT_EXPECTED[name], (name, br)
    return br


def predict_case_rows(name, args, out, rows):
    """The new matrix of a prediction case: the hard rows of the kept trees' rules (root rules of the LAST kept draw first) filled up to `rows` rows with
    new_rows; `rows` = 0: the hard rows alone; 1: the first of them.  Returns (x_new, number of root-rule triples in front, 0 if cut)."""
    draws = args.iter - args.warmup
    kept = out["kept_trees"]
    last = {k: v[kept["sample"] == draws - 1] for k, v in kept.items()}
    roots, _ = rule_list(last, 0)
    _, deeper = rule_list(kept, 200, seed=len(name))
    hard, n_root = hard_rows(args.x_bart, roots, deeper, seed=len(name))
    if rows == 1:
        return hard[:1].copy(), 0
    assert rows == 0 or rows > len(hard), (rows, len(hard))
    return (hard if rows == 0 else np.vstack([hard, new_rows(args.x_bart, rows - len(hard), seed=len(name))])), n_root


def check_prediction(lib, prefix, name, report=print):
    """One k_predict case, on `lib`: predict_bart(new rows) against the walk, predict_bart(training rows) against the stored bart.train columns, a
    sampler rebuilt from the exported state bit-equal to the live one.  Returns what the callers assert case-specific things on."""
    from stan4bart_amd.abi import StoredSampler
    build, rows, draws = PREDICT_CASES[name]
    args = build()
    assert args.iter - args.warmup == draws and args.keep_trees
    n, P = args.x_bart.shape
    binary = bool(args.is_binary)
    got = {}

    def then(s, out):
        x_new, n_root = predict_case_rows(name, args, out, rows)
        got["x_new"], got["n_root"] = x_new, n_root
        got["br"] = check_predict_branch(name, args, len(x_new))
        got["new"] = s.predict_bart(x_new)
        got["train"] = s.predict_bart(args.x_bart)
        st = StoredSampler(lib, prefix, s.export_bart_state())
        try:
            got["stored"] = st.predict_bart(x_new)
        finally:
            st.free()
    out = run_readout(lib, prefix, args, then=then, trace=False)
    x_new, br = got["x_new"], got["br"]
    assert got["new"].shape == (len(x_new), draws)
    ref, bound = walk_fits(out["kept_trees"], x_new, out["range"], binary)
    ratio = assert_within_bound(got["new"], ref, bound, name)
    # first and last element of every round of the grid-stride loop (element idx = draw * rows + row), explicitly
    flat_dev, flat_ref, flat_bound = got["new"].reshape(-1, order="F"), ref.reshape(-1, order="F"), bound.reshape(-1, order="F")
    total = flat_dev.size
    edges = sorted({e for r in range(br["rounds"]) for e in (r * br["per_round"], min((r + 1) * br["per_round"], total) - 1)})
    for e in edges:
        assert abs(flat_dev[e] - flat_ref[e]) <= BOUND_FACTOR * flat_bound[e], (name, "element", e, flat_dev[e], flat_ref[e])
    # the existing identity at its existing tolerance (the training fits are accumulated along the sweep, not summed per row)
    np.testing.assert_allclose(got["train"], out["sample"]["bart"]["train"], rtol=1e-9, atol=1e-9)
    assert np.array_equal(got["stored"], got["new"]), "a sampler rebuilt from the exported state predicts differently from the live one"
    report(f"k_predict {name}: {len(x_new)} rows x {draws} draws, T {args.n_trees}, P {P}, {br['grid']} workgroups, {br['rounds']} round(s), "
           f"threaded binning {br['threaded_binning']}; max |device - walk| / bound = {ratio:.3f}")
    return dict(args=args, out=out, got=got, ref=ref, bound=bound, ratio=ratio)


def assert_prediction_case(name, r):
    """What a prediction case asserts beyond agreement with the walk: that the shape it was built for really occurred."""
    kept, args, dev = r["out"]["kept_trees"], r["args"], r["got"]["new"]
    n_root = r["got"]["n_root"]
    if n_root:
        k = np.arange(n_root)
        assert np.array_equal(dev[3 * k], dev[3 * k + 2]), "a value just below a root cut and the cut value itself gave different fits"
    if name == "hard-rows":
        x = r["got"]["x_new"]
        assert n_root == args.n_trees >= 25 and len(x) > 3 * (n_root + 100) + 10 and np.isinf(x).any()          # every tree's root rule, deeper rules
        differed = assert_root_rule_rows(dev, n_root, dev.shape[1] - 1)
        print(f"hard rows: {differed} of {n_root} root-rule rows change between the cut value and the next double above it")
    if name == "deep":
        assert args.node_capacity == 1024 and nodes_per_tree(kept).max() > 128, int(nodes_per_tree(kept).max())
    if name == "quantile-cuts":
        rule = kept["var"] >= 0
        assert (kept["split"][rule & (kept["var"] == 0)] > 255).any(), "no kept rule uses a cut index beyond 255"
        assert not (kept["var"] == 1).any(), "a rule uses the predictor that has no cut"
    if name == "c5-200x140":
        assert args.n_trees == 200 and args.x_bart.shape[1] == 140 and kept["var"].max() >= 64
    if name == "binary":
        assert args.is_binary


def rows_for_test_fits(lib, prefix, args, n_test, seed=0):
    """Test rows that are not training rows: a first run of the chain without test rows gives its rules (test rows do not enter the chain), the hard rows
    of those come first, new_rows fill up; with fewer rows than hard rows: the first triple, the edge rows, then further triples.
    Returns (rows, the live trees of that first run: the caller asserts that the chain with the test rows ended on the same ones)."""
    a = copy.copy(args)
    a.x_test, a.keep_trees = None, True
    pre = run_readout(lib, prefix, a, trace=False)
    roots, _ = rule_list(pre["trees"], 0)
    _, deeper = rule_list(pre["kept_trees"], 200, seed=seed)
    hard, n_root = hard_rows(args.x_bart, roots, deeper, seed=seed)
    if n_test >= len(hard):
        return np.vstack([hard, new_rows(args.x_bart, n_test - len(hard), seed=seed)]), pre["trees"]
    order = np.r_[0:3, len(hard) - 10:len(hard), 3:len(hard) - 10]          # the first triple, the ten edge rows, the other triples
    return hard[order[:n_test]].copy(), pre["trees"]


def check_test_fits(lib, prefix, oracle_lib, name, report=print):
    """One k_test_fits_few / k_test_fits case on `lib`: the chain against the oracle (assert_chain_parity), the emitted bart.test columns against the walk
    (every kept draw where the trees are kept, else the last draw against the live trees), and bart.test against predict_bart of the same rows: equality."""
    from conftest import assert_chain_parity, run_chain
    build, n_test, T = TEST_FIT_CASES[name]
    base = build()
    assert base.n_trees == T
    br = check_test_fit_branch(name, n_test, T)
    x_test, pre_trees = rows_for_test_fits(lib, prefix, base, n_test, seed=len(name))
    assert x_test.shape[0] == n_test
    args = with_test_rows(base, x_test)
    binary = bool(args.is_binary)
    got = {}

    def then(s, out):
        if args.keep_trees:
            got["predict"] = s.predict_bart(x_test)
    b = run_readout(lib, prefix, args, then=then)
    for key in ("var", "value"):          # the rules the hard rows were built from are the chain's own
        assert np.array_equal(pre_trees[key], b["trees"][key]), "the test rows changed the chain"
    a = run_chain(oracle_lib, "orc_", args)
    assert_chain_parity(a, b)
    test = b["sample"]["bart"]["test"]
    assert test.shape == (n_test, args.iter - args.warmup)
    if args.keep_trees:
        ref, bound = walk_fits(b["kept_trees"], x_test, b["range"], binary)
        ratio = assert_within_bound(test, ref, bound, name)
        # k_test_fits(_few) and k_predict form the same sums in the same order from the same leaf values and apply the same scale expression
        assert np.array_equal(test, got["predict"]), (name, float(np.max(np.abs(test - got["predict"]))))
    else:
        ref, bound = walk_fits(b["trees"], x_test, b["range"], binary)
        ratio = assert_within_bound(test[:, -1:], ref, bound, name)
    report(f"k_test_fits{'_few' if br['kernel'] == 'few' else ''} {name}: {n_test} rows, T {T}, {br['grid']} workgroups, {br['rounds']} round(s), "
           f"{br['idle_rows']} idle row(s), {br['trees_per_lane']} tree(s) per lane/thread; max |device - walk| / bound = {ratio:.3f}")
    return dict(args=args, a=a, b=b, ratio=ratio)


def check_counts(lib, prefix, oracle_lib, name, report=print):
    """One k_var_counts / k_draw_k case on `lib`: the chain against the oracle (varcount exact, the k draws to the usual bar), varcount against a count of
    the rules of the flattened trees (exact), the read-out of the test rows against the walk."""
    from conftest import assert_chain_parity, run_chain
    build, P, T = COUNT_CASES[name]
    args = build()
    assert args.x_bart.shape[1] == P and args.n_trees == T and args.keep_trees
    br = counts_branch(P, T)
    assert (br["p_rounds"], br["t_rounds"]) == COUNT_EXPECTED[name] and br["k_rounds"] == br["t_rounds"], (name, br)
    got = {}

    def then(s, out):
        got["predict"] = s.predict_bart(args.x_test)
    b = run_readout(lib, prefix, args, then=then)
    draws = args.iter - args.warmup
    vc = b["sample"]["bart"]["varcount"]
    assert vc.shape == (P, draws)
    assert np.array_equal(vc, count_rules(b["kept_trees"], P, draws)), "varcount differs from the rules of the kept trees"
    assert np.array_equal(vc[:, -1], count_rules(b["trees"], P)), "the last varcount differs from the rules of the live trees"
    ref, bound = walk_fits(b["kept_trees"], args.x_test, b["range"])
    ratio = assert_within_bound(b["sample"]["bart"]["test"], ref, bound, name)
    assert np.array_equal(b["sample"]["bart"]["test"], got["predict"])
    a = run_chain(oracle_lib, "orc_", args)
    assert_chain_parity(a, b)
    if "chi" in name:
        assert "k" in b["sample"]["bart"] and np.std(b["sample"]["bart"]["k"]) > 0
    report(f"k_var_counts{' / k_draw_k' if 'chi' in name else ''} {name}: P {P} ({br['p_rounds']} round(s)), T {T} ({br['t_rounds']} round(s)); "
           f"highest predictor in use {int(np.flatnonzero(vc.sum(axis=1)).max())}; test rows: max |device - walk| / bound = {ratio:.3f}")
    return dict(args=args, a=a, b=b, varcount=vc)


def check_per_draw_scale(lib, prefix, report=print):
    """k_predict applies the response scale OF THE DRAW: warm-up (the scale moves) and sampling runs interleaved on one sampler, 3 + 2 four times; at
    least three distinct scales must occur among the 8 kept draws, and every draw is compared with the walk under its own scale."""
    from conftest import make_sampler
    args = _friedman(n=400, T=12, warmup=12, iter=20, ranef=False)
    s = make_sampler(lib, prefix, args)
    ranges, trains = [], []
    try:
        for _ in range(4):
            s.run(3, True)
            r = s.run(2, False)
            trains.append(r["bart"]["train"])
            ranges += [s.get_bart_data_range()] * 2
        kept = s.get_kept_trees()
        x_new, _ = predict_case_rows("scale", args, dict(kept_trees=kept), 0)
        x_new = np.vstack([x_new, new_rows(args.x_bart, 300, seed=5)])
        dev, dev_train = s.predict_bart(x_new), s.predict_bart(args.x_bart)
    finally:
        s.free()
    ranges = np.array(ranges)
    widths = np.unique(ranges[:, 1] - ranges[:, 0])
    assert len(widths) >= 3, f"the kept draws carry {len(widths)} distinct response scales: the case does not tell a per-draw scale from a shared one"
    assert dev.shape == (len(x_new), 8)
    ref, bound = walk_fits(kept, x_new, ranges)
    ratio = assert_within_bound(dev, ref, bound, "per-draw scale")
    np.testing.assert_allclose(dev_train, np.hstack(trains), rtol=1e-9, atol=1e-9)
    report(f"k_predict per-draw scale: {len(x_new)} rows x 8 draws, ranges {np.round(ranges[::2, 1] - ranges[::2, 0], 1).tolist()}; "
           f"max |device - walk| / bound = {ratio:.3f}")
    return ranges


def check_predictor_limit(lib, prefix):
    """A rule stores its predictor as int16_t (tree arrays, PackedNode::var): more than 32 767 predictors are refused at create, with a message."""
    import pytest
    from conftest import make_sampler
    args = _friedman(n=40, T=2, warmup=1, iter=2, ranef=False)
    args.x_bart = np.asfortranarray(np.random.default_rng(7).random((40, 32768)))
    with pytest.raises(RuntimeError, match="at most 32767 predictors"):
        make_sampler(lib, prefix, args)
