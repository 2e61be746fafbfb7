"""The Stan -> BART hand-off ALONE (k_offset_rescale; k_param_mean + k_set_sigma + k_scale + k_rescale; k_rescale_binary; the create path; k_param_mean into
s.e for get_parametric_mean — stan4bart_amd/csrc/dev_hip.hip) through the test entry s4b_test_hand_off, and an audit of the shared residual against its
own trees: the reference, the bounds, the branch functions and the case builders shared by tests/test_gpu_handoff.py (libs4b.so on the GPU) and its CPU
twin tests/test_handoff.py (the emulated device layer and the oracle).

The reference is a numpy longdouble model written from DESIGN.md section 4.  It shares no code with the kernels, the emulation or the oracle; it reads the
inputs of create (X, the CSR triplet of Z, the user's offset, y) and the state blobs (conftest.StateView) before and after one hand-off:
    eta = X beta + Z b [+ user]          with the terms the sampler's offset type names (offset_flags)
    min, max of y - eta;  range = max - min
    with a scale update:   shift = (min0 + range0 / 2 - min - range / 2) / T,  mu' = (range0 mu + shift) / range,  F' = (range0 F + T shift) / range
    R' = yNew - F',  yNew = (y - eta - min) / range - 1/2
    binary response:       latent' = latent + (offset - eta) (latent + offset invariant), R moved by the same amount: the total fits stay.

Bounds, u = 2^-53; every comparison with the model allows BOUND_FACTOR = 4 times its bound (the long-double reference's own roundings and the conversion
to double, as in readout_cases.py).  `m` is the number of terms of an entry, A the sum of their absolute values.
  offsets       The device adds m products one after the other: every term meets at most m roundings (its product, the sums after it), each relative to a
                partial sum no larger than A: |offset - eta| <= m u A.  An entry without a term is exactly 0.
  min, max      No bound: bit-equal to min / max of (y - offset) formed in double from the offsets the device returned (any order of fmin / fmax gives the
                same result), range bit-equal to max - min; without an update the three are the bits they were.
  sigmaData     The device stores sigma itself.  The oracle keeps sigma / range and the blob multiplies back, and a scale update divides and multiplies once
                more: 4 roundings, |sigmaData - sigma| <= 4 u sigma.
  leaf values   S = (min0 + range0 / 2) - min - range / 2 is three sums of partial results no larger than M = |min0| + range0 / 2 + |min| + range / 2, the
                division by T rounds once more: |shift error| <= 4 u M / T.  range0 mu rounds once, adding the shift rounds once relative to at most
                |range0 mu| + |shift|, the division once relative to the result:
                    |mu' error| <= u ((4 M / T + 2 |range0 mu| + |shift|) / range + |mu'|).
                Without an update the leaf values are the bits they were.
  total fits    The blob holds F = yRescaled - R, formed on the host by the kernels' own expression.  With an update the device forms F = yOld - R (the
                blob's F0, bit for bit), T * shift (the shift's error times T, one rounding), range0 F (one), their sum (one), the quotient (one),
                R' = yNew - F' (one, relative to |R'|), and the blob forms yNew - R' (one, relative to |F'|):
                    |F' error| <= u ((4 M + 2 |S| + 2 |range0 F0|) / range + 2 |F'| + |R'|).
                The oracle sums its T rescaled tree fits instead: the T leaf-value bounds and T roundings of the sum are added for it.
                Without an update: R' = fl(yNew - F0) and the blob's fl(yNew - R') differ from F0 by one rounding relative to |R'| and one relative to |F|:
                    |F' - F0| <= C_KEEP u max(|R|, |F|), C_KEEP = 2 (both states' R and F in the max).
                Binary: d = fl(latent' - latent), R' = fl(R + d), the blob's fl(latent' - R') against fl(latent - R): one rounding each relative to |d|,
                |R'|, |F'|, |F0|: C_KEEP_BINARY = 4 with |d| in the max; latent' + eta against latent + offset: u (|offset - eta| + |latent'|).
Everything else in the blob (NUTS point, metric, adaptation, both generators, tree structure, node counts, the modeled k) is bit-identical.

The audit (audit_state) checks, for every observation and every tree, from get_state / get_trees / get_leaf_assignment alone:
  * the leaf assignment equals the routing of the RAW predictor rows through the flattened trees (readout_cases.walk_leaves), exactly;
  * the leaf counts equal the histogram of the assignment;
  * the total fits equal the sum of the assigned leaf values (long double) within AUDIT bound = u * M * W, W the weighted number of roundings since
    create and M the largest of |R|, |F|, sum_t |mu_t| (and |latent| for a binary response) over all observations at the audit points so far:
      tree update        R <- (R + muOld) - muNew: 2 roundings of intermediates no larger than |R| + |mu| <= 2 M                       weight 4
      hand-off           F = yOld - R, R' = yNew - F: 2 (binary: d and R + d, |d| <= 2 M: 4)                                        weight 2 / 4
      scale update       F side: range0 F, T shift, their sum, the quotient (the shift's own error is common to both sides): 4; leaf side: 3 per tree;
                         each relative to intermediates the update amplifies by a = max(1, (range0 M + |S|) / (range M)) — the hand-off cases pass the
                         a they measured from the blobs; a free run is charged a = 4 per update, which is ASSUMED, NOT MEASURED: the scale
                         between two updates inside run() cannot be read through the existing entries, so nothing asserts that the range moves
                         by less than a factor of 2 from one update to the next (what a = 4 rests on, the offsets being the model's own
                         parametric mean).  audited_run asserts what the audit points do show — a sampling phase leaves min and range bit-identical,
                         so no update goes uncharged there — and reports the range ratio across the warm-up           weight (3 T + 4) a
      latent draw        F = latent - R, R' = latent' - F                                                                             weight 2
      create / blob      k_assign_leaves subtracts the T leaf values one after the other (T roundings of at most 2 M), the blob forms yRescaled - R: 1
                                                                                                                                     weight 2 T + 1
    The bound is a worst case on purpose (every rounding at its maximum and with the same sign).  On the emulation a Friedman chain (n = 2 000, 20 trees,
    400 iterations, 8 020 tree updates) drifts 5.1e-15, a binary chain (n = 1 000, 4 020 updates) 2.3e-14; a tree update folded into the wrong leaf, a
    stale leaf plane or a leaf value that missed a rescaling shows at 1e-3 ... 1."""
import os
import re
import zlib

import numpy as np

from readout_cases import BOUND_FACTOR, U, bound_ratio, tree_starts, walk_leaves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_HIP = os.path.join(ROOT, "stan4bart_amd", "csrc", "dev_hip.hip")
LD = np.longdouble
C_KEEP, C_KEEP_BINARY = 2.0, 4.0
OFFSET_TYPES = ["default", "fixef", "ranef", "bart", "parametric"]
FREE_RUN_AMPLIFICATION = 4.0      # assumed, not measured (module docstring, "scale update")


# ---- which route and which geometry a shape selects ------------------------------------------------------------------------------------------------------
def handoff_limits(src_path=DEV_HIP):
    """The constants that decide the route and the geometry of a hand-off, READ from dev_hip.hip; the statements restated by hand_off_route and
    geometry are asserted to still be there, so that a moved threshold or a reshaped launch fails here instead of quietly moving the cases."""
    src = open(src_path).read()
    lim = dict(block=int(re.search(r"constexpr int BLOCK = (\d+);", src).group(1)))
    m = re.search(r"if \(!binary_ && K_ \+ q_ <= (\d+)\) \{\s*pend_\.fixed = fixed;", src)
    assert m, "offset_from_params no longer holds the call for the one-launch form under `!binary_ && K_ + q_ <= ...`"
    lim["inline"] = int(m.group(1))
    m = re.search(r"struct OffsetArgs \{ int32_t fixed, random, addUser, pad; double sigmaData; double par\[(\d+)\]; \};", src)
    assert m and int(m.group(1)) == lim["inline"], "OffsetArgs::par no longer has one slot per inlined coefficient"
    assert re.search(r"if \(threadIdx\.x < %d\) par\[threadIdx\.x\] = o\.par\[threadIdx\.x\];" % lim["inline"], src)
    assert "if (pendOffset_ && pendSigma_ && !update) {" in src, "rescale() no longer chooses the one-launch form by `pendOffset_ && pendSigma_ && !update`"
    assert "const int64_t nQuads = (n_ + 3) / 4;" in src
    m = re.search(r"a\.grid = \(int\)std::min<int64_t>\((\d+), std::max<int64_t>\(1, \(nQuads \+ BLOCK - 1\) / BLOCK\)\);", src)
    assert m, "the a.grid formula changed"
    lim["grid_cap"] = int(m.group(1))
    assert "gridN_ = a.grid;" in src
    # the launches of the three routes and of the create path, with their geometry
    for stmt in ("hipLaunchKernelGGL(k_offset_rescale, dim3(gridN_), dim3(BLOCK), 0, stream_, a_, s_, pend_); ++launches_;",
                 "hipLaunchKernelGGL(k_param_mean, dim3(gridN_), dim3(BLOCK), 0, stream_, a_, s_, pend_.fixed, pend_.random, pend_.addUser, 0, a_.offNew); ++launches_;",
                 "hipLaunchKernelGGL(k_param_mean, dim3(gridN_), dim3(BLOCK), 0, stream_, a_, s_, fixed, random, addUser, 0, a_.offNew); ++launches_;",
                 "if (pendSigma_) { pendSigma_ = false; hipLaunchKernelGGL(k_set_sigma, dim3(1), dim3(1), 0, stream_, a_, pend_.sigmaData); ++launches_; }",
                 "hipLaunchKernelGGL(k_set_sigma, dim3(1), dim3(1), 0, stream_, a_, s); ++launches_;",
                 "hipLaunchKernelGGL(k_scale, dim3(1), dim3(BLOCK), 0, stream_, a_, s_, update ? 1 : 0, gridN_); ++launches_;",
                 "hipLaunchKernelGGL(k_rescale, dim3(gridN_), dim3(BLOCK), 0, stream_, a_, update ? 1 : 0); ++launches_;",
                 "hipLaunchKernelGGL(k_rescale_binary, dim3(gridN_), dim3(BLOCK), 0, stream_, a_); ++launches_;",
                 "hipLaunchKernelGGL(k_param_mean, dim3(gridN_), dim3(BLOCK), 0, stream_, a_, s_, 1, 1, 0, 0, s_.e); ++launches_;"):
        assert stmt in src, stmt
    # k_scale: one workgroup of BLOCK threads goes round the partials and round the T * nc leaf slots
    assert "for (int b = threadIdx.x; b < gridUsed; b += blockDim.x) { mn = fmin(mn, s.mmPart[b]); mx = fmax(mx, s.mmPart[a.grid + b]); }" in src
    assert "for (size_t k = threadIdx.x; k < m; k += blockDim.x) a.mu[k] = (sc.range0 * a.mu[k] + sc.shiftPerTree) / sc.range;" in src
    assert "for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * BLOCK) {" in src
    return lim


def _ceil(a, b):
    return -(-a // b)


def hand_off_route(K, q, binary, update, lim=None):
    """Kernel launches of one hand-off: 1 (k_offset_rescale), 4 (k_param_mean + k_set_sigma + k_scale + k_rescale) or 2 (binary: k_param_mean +
    k_rescale_binary)."""
    L = lim or handoff_limits()
    if binary:
        return 2
    return 1 if (K + q <= L["inline"] and not update) else 4


def geometry(n, T=1, nc=256, lim=None):
    """grid (workgroups of every O(N) kernel), trips of the grid-stride loop (of the busiest thread), whether the last trip is ragged, rounds of k_scale's
    fold of the partials and of its loop over the T * nc leaf slots."""
    L = lim or handoff_limits()
    B = L["block"]
    grid = min(L["grid_cap"], max(1, _ceil(_ceil(n, 4), B)))
    per = grid * B
    return dict(block=B, grid=grid, trips=_ceil(n, per), ragged=n % per != 0, fold_rounds=_ceil(grid, B), slot_rounds=_ceil(T * nc, B))


def obs_index(workgroup, thread, trip, n, lim=None):
    """Observation that `thread` of `workgroup` handles on its `trip`-th round of the grid-stride loop."""
    g = geometry(n, lim=lim)
    i = trip * g["grid"] * g["block"] + workgroup * g["block"] + thread
    assert 0 <= workgroup < g["grid"] and 0 <= thread < g["block"] and i < n, (workgroup, thread, trip, n)
    return i


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------------
def offset_flags(args):
    """(fixed, random, user): the terms of BART's offset under the sampler's offset type (reference src/init.cpp:762-795)."""
    if args.offset is None:
        return True, True, False
    return {"default": (True, True, True), "bart": (True, True, False), "ranef": (True, False, True), "fixef": (False, True, True),
            "parametric": (False, False, True)}[OFFSET_TYPES[args.offset_type]]


def eta_model(args, beta, b, flags=None):
    """(eta in long double, its bound per entry) for coefficients beta, b."""
    fixed, random, user = offset_flags(args) if flags is None else flags
    n = len(args.y)
    eta, mag, cnt = np.zeros(n, LD), np.zeros(n, LD), np.zeros(n, np.int64)
    X = np.asarray(args.X, dtype=np.float64).reshape(n, -1)
    if fixed:
        for k in range(X.shape[1]):
            t = X[:, k].astype(LD) * LD(beta[k])
            eta += t; mag += np.abs(t); cnt += 1
    u = np.asarray(args.u, dtype=np.int64)
    if random and len(np.asarray(args.w)):
        rows = np.repeat(np.arange(n), np.diff(u))
        t = np.asarray(args.w, dtype=np.float64).astype(LD) * np.asarray(b, dtype=np.float64)[np.asarray(args.v, dtype=np.int64)].astype(LD)
        np.add.at(eta, rows, t); np.add.at(mag, rows, np.abs(t)); cnt += np.diff(u)
    if user:
        t = np.asarray(args.offset, dtype=np.float64).astype(LD)
        eta += t; mag += np.abs(t); cnt += 1
    return eta, (cnt * U * mag).astype(np.float64)


def _ratio(device, reference, bound, what, report):
    r = bound_ratio(device, reference, bound)
    report[what] = max(report.get(what, 0.0), r)
    assert r <= BOUND_FACTOR, f"{what}: |device - model| is {r:.3g} x the derived bound (allowed: {BOUND_FACTOR:g})"
    return r


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b, what):
    assert np.array_equal(_bits(a), _bits(b)), f"{what}: not bit-identical"


def rescaled_response(args, sv):
    """yRescaled (double, the kernels' own expression) and R = yRescaled - F of a state; binary: the latents and R = latent - F."""
    F = sv.get("total_fits")
    if sv.binary:
        lat = sv.get("latents")
        return lat, lat - F
    mn, _, rng, _ = sv.get("scale")
    yr = (np.asarray(args.y, dtype=np.float64) - sv.get("offset") - mn) / rng - 0.5
    return yr, yr - F


def state_view(s):
    """StateView of a sampler's state (the 16 bytes that latent mode 1 appends — key and draw index of the parallel latents — are not part of its layout)."""
    from conftest import StateView
    blob = s.get_state()
    return StateView(blob[:-16] if s.get_latent_mode() == 1 else blob)


UNTOUCHED = ("q", "inv_metric", "wm", "wm2", "nuts", "last", "win", "ecuyer", "r_rng")


def check_hand_off(args, before, after, beta, b, sigma, update, impl, report):
    """One hand-off under the model: `before` / `after` are StateViews around s.test_hand_off(beta, b, sigma, update).  `impl`: "s4b", "emu" or "orc"
    (the oracle sums its tree fits after an update: see the module docstring).  Largest ratios to the bounds go into `report`.  Returns the amplification
    a of this scale update (1 without one) for the audit's ledger."""
    y = np.asarray(args.y, dtype=np.float64)
    T = before.T
    # -- everything the hand-off has no business with
    for k in UNTOUCHED:
        assert np.array_equal(before.get(k), after.get(k)), f"{k} changed across a hand-off"
    assert _bits([before.k])[0] == _bits([after.k])[0], "the modeled k changed across a hand-off"
    for t, ((n0, m0), (n1, m1)) in enumerate(zip(before.trees, after.trees)):
        assert np.array_equal(n0, n1), f"tree {t}: structure or node counts changed across a hand-off"
    # -- offsets
    eta, eta_bound = eta_model(args, beta, b)
    off0, off1 = before.get("offset"), after.get("offset")
    _ratio(off1, eta, eta_bound, "offset", report)
    sc0, sc1 = before.get("scale"), after.get("scale")
    F0, F1 = before.get("total_fits"), after.get("total_fits")
    mu0 = np.concatenate([m for _, m in before.trees])
    mu1 = np.concatenate([m for _, m in after.trees])
    if before.binary:
        _same_bits(sc0, sc1, "the scale of a binary response")
        _same_bits(mu0, mu1, "leaf values (binary)")
        lat0, lat1 = before.get("latents"), after.get("latents")
        d = off0.astype(LD) - off1.astype(LD)
        _ratio(lat1, lat0.astype(LD) + d, (U * (np.abs(d) + np.abs(lat1))).astype(np.float64), "latent + offset", report)
        R0, R1 = lat0 - F0, lat1 - F1
        mag = np.maximum.reduce([np.abs(R0), np.abs(R1), np.abs(F0), np.abs(F1), np.abs(lat1 - lat0)])
        r = bound_ratio(F1, F0, C_KEEP_BINARY * U * mag)
        report["fits kept"] = max(report.get("fits kept", 0.0), r)
        assert r <= 1.0, f"binary hand-off: the total fits moved by {r:.3g} x C_KEEP_BINARY u max(|R|, |F|, |d|)"
        return 1.0
    _ratio(sc1[3:4], np.array([sigma], LD), np.array([4.0 * U * sigma]), "sigmaData", report)
    if impl != "orc":
        assert sc1[3] == sigma, "the device stores sigma itself"
    v = y - off1                                              # (double, from the offsets the device returned)
    if not update:
        _same_bits(sc0[:3], sc1[:3], "min / max / range without a scale update")
        _same_bits(mu0, mu1, "leaf values without a scale update")
        _, R0 = rescaled_response(args, before)
        _, R1 = rescaled_response(args, after)
        mag = np.maximum.reduce([np.abs(R0), np.abs(R1), np.abs(F0), np.abs(F1)])
        r = bound_ratio(F1, F0, C_KEEP * U * mag)
        report["fits kept"] = max(report.get("fits kept", 0.0), r)
        assert r <= 1.0, f"hand-off without a scale update: the total fits moved by {r:.3g} x C_KEEP u max(|R|, |F|)"
        return 1.0
    mn, mx = float(np.min(v)), float(np.max(v))
    _same_bits([sc1[0], sc1[1], sc1[2]], [mn, mx, mx - mn], "min / max / range of y - offset")
    min0, range0, rng = LD(sc0[0]), LD(sc0[2]), LD(sc1[2])
    S = (min0 + range0 / 2) - LD(mn) - rng / 2
    M = abs(min0) + range0 / 2 + abs(LD(mn)) + rng / 2
    shift = S / T
    mu_ref = (range0 * mu0.astype(LD) + shift) / rng
    mu_bound = U * ((4 * M / T + 2 * np.abs(range0 * mu0.astype(LD)) + abs(shift)) / rng + np.abs(mu_ref))
    # (the oracle recovers a leaf's value from the fit of its first observation: a leaf without observations has none there, and its slot is not compared)
    seen = np.concatenate([nd[nd[:, 0] < 0, 1] for nd, _ in after.trees]) > 0 if impl == "orc" else np.ones(len(mu1), dtype=bool)
    _ratio(mu1[seen], mu_ref[seen], mu_bound.astype(np.float64)[seen], "leaf values", report)
    F_ref = (range0 * F0.astype(LD) + S) / rng
    y_new = (y.astype(LD) - off1.astype(LD) - LD(mn)) / rng - LD(0.5)
    F_bound = U * ((4 * M + 2 * abs(S) + 2 * np.abs(range0 * F0.astype(LD))) / rng + 2 * np.abs(F_ref) + np.abs(y_new - F_ref))
    if impl == "orc":
        F_bound = F_bound + T * float(mu_bound.max()) + T * U * T * float(np.abs(mu_ref).max())
    _ratio(F1, F_ref, F_bound.astype(np.float64), "total fits", report)
    Mb = max(float(np.abs(F0).max()), float(np.abs(mu0).max()), 0.5)
    Ma = max(float(np.abs(F1).max()), float(np.abs(mu1).max()), 0.5)
    return max(1.0, float((range0 * Mb + abs(S)) / (rng * Ma)))


def check_parametric_mean(args, s, row, names, report):
    """get_parametric_mean() against X beta + Z b of the Stan row `row` (the last draw run() returned, `names` its parameter names)."""
    beta = np.array([row[i] for i, nm in enumerate(names) if nm.startswith("beta.")])
    b = np.array([row[i] for i, nm in enumerate(names) if re.fullmatch(r"b\.\d+", nm)])
    eta, bound = eta_model(args, beta, b, flags=(True, True, False))
    pm = s.get_parametric_mean()
    assert np.abs(pm).max() > 0
    return _ratio(pm, eta, bound, "parametric mean", report)


# ---- the audit ---------------------------------------------------------------------------------------------------------------------------------------
class Ledger:
    """What has rounded the residual since create (the audit's bound is linear in it) and the largest magnitude seen at the audit points."""

    def __init__(self, T, binary, thin=1):
        self.T, self.binary = T, binary
        self.hand_offs = 0
        self.scale_updates = 0.0      # sum of the amplifications a
        self.latent_draws = thin if binary else 0          # (the sweep inside create)
        self.M = 0.0

    def run(self, iters, warmup, thin=1, results_type=0):
        """A run() of `iters` iterations: one hand-off each, scale updates by run()'s own schedule, a latent draw per sweep of a binary response."""
        if results_type in (0, 2):
            self.hand_offs += iters
            if warmup:
                self.scale_updates += FREE_RUN_AMPLIFICATION * sum(1 for it in range(iters) if it % (1 << (8 * it // iters)) == 0)
        if self.binary and results_type in (0, 1):
            self.latent_draws += iters * thin

    def hand_off(self, update, amplification=1.0):
        self.hand_offs += 1
        if update:
            self.scale_updates += amplification

    def weight(self, tree_updates):
        T = self.T
        w = 4.0 * tree_updates + (4.0 if self.binary else 2.0) * self.hand_offs + (3.0 * T + 4.0) * self.scale_updates + 2.0 * self.latent_draws
        return w + 2.0 * T + 1.0


def audit_state(s, x_raw, args, ledger, report=None, what="audit"):
    """The three invariants of the module docstring on sampler `s` (any implementation), from get_state, get_trees, get_leaf_assignment and the tree
    updates of get_counters.  `x_raw`: the raw predictor rows create was given.  Returns the drift max |F - sum of assigned leaf values|."""
    sv = state_view(s)
    trees = s.get_trees()
    F = sv.get("total_fits")
    n, T = sv.n, sv.T
    var, value, cnt = trees["var"], trees["value"], trees["n"]
    starts, end = tree_starts(trees)
    assert len(starts) == T
    leaf_rank = np.cumsum(var < 0) - 1                       # rank among all leaf entries of the list
    total, mabs = np.zeros(n, LD), np.zeros(n, LD)
    for a, st, pos in walk_leaves(trees, x_raw):
        en = int(end[st])
        walked = (leaf_rank[pos] - leaf_rank[st:en][var[st:en] < 0][0]).astype(np.int32)          # DFS rank of the reached leaf within its tree
        assigned = s.get_leaf_assignment(a)
        bad = np.flatnonzero(walked != assigned)
        assert not len(bad), f"{what}: tree {a}: the leaf assignment of {len(bad)} observation(s) differs from the routing of their rows (first: {int(bad[0])})"
        leaves = np.flatnonzero(var[st:en] < 0) + st
        hist = np.bincount(walked, minlength=len(leaves))
        assert np.array_equal(hist, cnt[leaves]), f"{what}: tree {a}: the leaf counts differ from the histogram of the assignment"
        total += value[pos].astype(LD); mabs += np.abs(value[pos]).astype(LD)
    _, R = rescaled_response(args, sv)
    mags = [np.abs(R).max(), np.abs(F).max(), float(mabs.max())] + ([np.abs(sv.get("latents")).max()] if sv.binary else [])
    ledger.M = max(ledger.M, float(max(mags)))
    bound = U * ledger.M * ledger.weight(int(s.get_counters()[1]))
    drift = float(np.abs(F.astype(LD) - total).max())
    assert np.isfinite(drift)
    if report is not None:
        report["audit"] = max(report.get("audit", 0.0), drift / bound)
    assert drift <= bound, f"{what}: the total fits differ from the sum of the assigned leaf values by {drift:.3g}, bound {bound:.3g}"
    return drift


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------------
def _limits_n():
    L = handoff_limits()
    one = 4 * L["block"]                                      # the last n of one workgroup (a quad per thread)
    return L, one


def case_table():
    """name -> keywords of build_case.  Every case is named for the branch it is for; HANDOFF_EXPECTED (tests/test_handoff.py) pins what geometry and
    which routes it must select."""
    L, one = _limits_n()
    B, cap = L["block"], L["grid_cap"]
    many = B * one + 1                                        # the first n with more than `B` workgroups: k_scale's threads go round the partials
    beyond = cap * one + 3 * B + 41                           # beyond the cap: a fifth trip, ragged
    C = {}
    # n at the geometry's edges (n = 1 as a binary response: a continuous response of one observation has range 0, and (y - min) / range is 0 / 0 in the
    # reference as well)
    C["n-1"] = dict(n=1, binary=True, terms=[(1, 0)], K=1)
    C["n-3"] = dict(n=3, terms=[(2, 0)], K=1)
    for n in (B - 1, B, B + 1, one, one + 1, many, beyond):
        C["n-%d" % n] = dict(n=n)
    # extremes of y - eta planted at chosen places: (max at, min at) as (workgroup, thread, trip) or an index
    small, big = 2 * one + 452, many + 855                    # 3 workgroups / 257 workgroups, 4 trips each, ragged
    C["ext-first-last"] = dict(n=small, plant=("first", "last"))
    C["ext-last-first"] = dict(n=small, plant=("last", "first"))
    C["ext-lane63-wave3"] = dict(n=small, plant=((1, B - 1, 0), (2, B - 1, 2)))
    C["ext-workgroup-256"] = dict(n=big, plant=((B, 0, 0), (B, B - 1, 1)))
    C["ext-last-workgroup"] = dict(n=big, plant=(("last-workgroup", 7, 0), ("last-workgroup", 3, 3)))
    C["ext-tie"] = dict(n=big, plant="tie")
    # K and q
    C["K0-q6"] = dict(n=1500, K=0, terms=[(6, 0)])
    C["q0-K3"] = dict(n=1500, K=3, terms=[])
    C["K12-q52"] = dict(n=1500, K=12, terms=[(52, 0)])          # K + q = 64: the last shape whose coefficients travel in the kernel arguments
    C["K12-q53"] = dict(n=1500, K=12, terms=[(53, 0)])          # 65: the first that takes four launches for every hand-off
    # rows of Z
    C["z-fixed-3"] = dict(n=1500, terms=[(5, 1), (4, 0)])
    C["z-ragged"] = dict(n=1500, terms=[(5, 1), (3, 1)], ragged=True)
    # offset types (user offsets of 1e3 times the response's range), several workgroups and trips
    C["off-none"] = dict(n=small)
    for ot in OFFSET_TYPES:
        C["off-" + ot] = dict(n=small, offset_type=ot)
    # scale updates that change the range by 1e-6 and 1e6 (the cases above leave it nearly the same)
    C["range-shrink-grow"] = dict(n=small, y_mode="shrink")
    C["range-grow-shrink"] = dict(n=small, y_mode="grow")
    # tree counts and capacities: k_scale's loop over T * nc leaf slots
    C["T1"] = dict(n=1500, T=1)
    C["T200-nc256"] = dict(n=1500, T=200)
    C["T200-nc1000"] = dict(n=1500, T=200, nc=1000)
    # binary
    C["binary-small"] = dict(n=200, binary=True)
    C["binary-3-workgroups"] = dict(n=small, binary=True)
    return C


def _place(p, n):
    if p == "first":
        return 0
    if p == "last":
        return n - 1
    if isinstance(p, tuple):
        w, t, r = p
        return obs_index(geometry(n)["grid"] - 1 if w == "last-workgroup" else w, t, r, n)
    return int(p)


_CACHE = {}


def build_case(name, spec=None):
    """Sampler arguments and the two hand-offs of a case: dict(args, hand_offs = [(beta, b, sigma), (beta, b, sigma)], planted = [(imax, imin) or None]
    per hand-off, pre = warm-up iterations run before the first hand-off).  Where a chain starts is not the subject: bart_offset_init is 0 and
    sigma_init 1 (no least-squares fit at n = 1e6), the tree prior is deep (base 0.99, power 0.8) so that trees from the prior have real depth."""
    if spec is None and name in _CACHE:
        return _CACHE[name]
    import stan4bart_amd.fit as fit
    from stan4bart_amd import GroupTerm
    sp = dict(K=2, terms=[(5, 0)], ragged=False, T=3, nc=None, binary=False, offset_type=None, plant=None, y_mode=None)
    sp.update(case_table()[name] if spec is None else spec)
    n, K = sp["n"], sp["K"]
    g = np.random.default_rng(zlib.crc32(name.encode()))
    p = 3
    xb = np.empty((n, p), order="F")
    for j in range(p):
        xb[:, j] = g.random(n)
    X = g.standard_normal((n, K)) if K else None
    y = 10.0 * np.sin(np.pi * xb[:, 0] * xb[:, 1]) + 5.0 * xb[:, 2] + g.standard_normal(n)
    groups = []
    for t, (levels, n_slopes) in enumerate(sp["terms"]):
        lev = (g.permutation(n) % levels) + 1
        slopes = g.standard_normal((n, n_slopes)) if n_slopes else None
        y = y + g.standard_normal(levels)[lev - 1] * 0.7
        groups.append(GroupTerm(lev, slopes, "g.%d" % (t + 1)))
    if sp["binary"]:
        y = (y > np.median(y)).astype(np.float64) if n > 1 else np.ones(1)
    user = None
    if sp["offset_type"] is not None:
        user = 1e3 * (float(np.ptp(y)) if not sp["binary"] else 1.0) * g.standard_normal(n)
    full_init = fit.init_fit
    fit.init_fit = lambda y_, Xc_, groups_, n_, binary_: (np.zeros(n_), 1.0)
    try:
        args = fit.make_sampler_args(y, xb, X=X, groups=groups, family="binomial" if sp["binary"] else "gaussian", iter=8, warmup=4,
                                     offset=user, offset_type=sp["offset_type"] or "default",
                                     bart_args={"n.trees": sp["T"], "n.cuts": 100, "base": 0.99, "power": 0.8})
    finally:
        fit.init_fit = full_init
    if sp["nc"]:
        args.node_capacity = sp["nc"]
    q = int(sum(int(a) * int(c) for a, c in zip(args.p, args.l)))
    if sp["ragged"]:
        # drop the explicit zeros of the last slope column (a third of its rows) AND every entry of a fifth of the rows: rows of 0, 3 and 4 stored entries
        z = int(sum(args.p))
        w2 = np.asarray(args.w).reshape(n, z).copy()
        w2[g.random(n) < 1.0 / 3.0, z - 1] = 0.0
        w2[g.random(n) < 0.2, :] = 0.0
        keep = w2 != 0.0
        assert (~keep.any(axis=1)).any() and keep.all(axis=1).any()
        args.u = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
        args.v = np.asarray(args.v).reshape(n, z)[keep].copy()
        args.w = w2[keep].copy()
    Xc = np.asarray(args.X, dtype=np.float64).reshape(n, -1)
    hand_offs = []
    beta = g.uniform(-1.0, 1.0, K)
    b = 0.7 * g.standard_normal(q)
    for h, sigma in enumerate((0.7, 1.3)):
        hand_offs.append((beta.copy(), b.copy(), sigma))
        beta = beta + 0.2 * g.uniform(-1.0, 1.0, K)
        b = b + 0.1 * g.standard_normal(q)
    planted = [None, None]
    if sp["y_mode"] in ("shrink", "grow"):
        # the response is 1e3 * X[:, 0] up to 1e-3: a hand-off whose beta[0] is 1e3 leaves a millionth of the range, one whose beta is 0 restores it
        args.y = 1e3 * Xc[:, 0] + 1e-3 * g.standard_normal(n)
        zero, cancel = np.zeros(K), np.r_[1e3, np.zeros(K - 1)]
        order = (cancel, zero) if sp["y_mode"] == "shrink" else (zero, cancel)
        if sp["y_mode"] == "grow":                           # create must see the small range first: the user-free offset cannot, so the response starts small
            args.y = 1e-3 * g.standard_normal(n)
            order = (-cancel, zero)
        hand_offs = [(order[0], 0.0 * hand_offs[0][1], 0.7), (order[1], 0.0 * hand_offs[1][1], 1.3)]
    if sp["plant"] == "tie":
        # coefficients of exactly 0: y - eta is y itself, and the same largest (smallest) value stands at two places far apart
        hand_offs = [(0.0 * bt, 0.0 * bb, sg) for bt, bb, sg in hand_offs]
        yy = np.array(args.y)
        hi, lo = float(yy.max()) + 3.0, float(yy.min()) - 3.0
        gm = geometry(n)
        places = (obs_index(0, 5, 0, n), obs_index(gm["grid"] - 1, 9, 1, n), obs_index(1, 63, 0, n), obs_index(gm["block"], 64, 2, n))
        yy[places[0]] = yy[places[1]] = hi
        yy[places[2]] = yy[places[3]] = lo
        args.y = yy
        planted = [((places[0], places[1]), (places[2], places[3]))] * 2
    elif sp["plant"] is not None:
        imax, imin = _place(sp["plant"][0], n), _place(sp["plant"][1], n)
        eta1 = eta_model(args, hand_offs[0][0], hand_offs[0][1])[0].astype(np.float64)
        yy = np.array(args.y)
        spread = float(np.ptp(yy - eta1))
        yy[imax] = eta1[imax] + float((yy - eta1).max()) + spread
        yy[imin] = eta1[imin] + float((yy - eta1).min()) - spread
        args.y = yy
        planted = [((imax,), (imin,))] * 2
    # (two warm-up iterations first where they cost nothing: trees the sweep has worked on, a Stan row.  Not where create must see the response's own range.)
    out = dict(name=name, args=args, hand_offs=hand_offs, planted=planted, pre=2 if 10 <= n <= 5000 and not sp["y_mode"] else 0, K=K, q=q, spec=sp)
    if spec is None:
        _CACHE[name] = out
    return out


def run_case(lib, prefix, name, update, report, expect_route=True):
    """One case on one implementation: [warm-up,] state, hand-off, state, model; again from the state the first left; the audit after each; the route from
    the launch counter where the implementation has one (libs4b.so).  Returns a dict of what the callers assert case-specific things on."""
    from conftest import StateView, make_sampler
    case = build_case(name)
    args = case["args"]
    impl = prefix.rstrip("_")
    s = make_sampler(lib, prefix, args)
    out = dict(case=case, launches=[], amplification=[])
    try:
        ledger = Ledger(args.n_trees, bool(args.is_binary), args.n_thin)
        if case["pre"]:
            s.run(case["pre"], True)
            ledger.run(case["pre"], True)
        before = StateView(s.get_state())
        out["nodes"] = max(len(nd) for nd, _ in before.trees)
        out["scales"] = [before.get("scale")]
        for h, (beta, b, sigma) in enumerate(case["hand_offs"]):
            c0 = int(s.get_counters()[2])
            s.test_hand_off(beta, b, sigma, update)
            out["launches"].append(int(s.get_counters()[2]) - c0)
            after = StateView(s.get_state())
            a = check_hand_off(args, before, after, beta, b, sigma, update, impl, report)
            out["amplification"].append(a)
            ledger.hand_off(update, a)
            if case["planted"][h] is not None:
                v = np.asarray(args.y, dtype=np.float64) - after.get("offset")
                imax, imin = case["planted"][h]
                assert set(np.flatnonzero(v == v.max()).tolist()) == set(imax) and set(np.flatnonzero(v == v.min()).tolist()) == set(imin), \
                    f"{name}: the extremes of y - offset are not at the planted places"
            audit_state(s, args.x_bart, args, ledger, report, what=f"{name} after hand-off {h + 1}")
            out["scales"].append(after.get("scale"))
            before = after
        if impl == "s4b" and expect_route:
            want = hand_off_route(case["K"], case["q"], bool(args.is_binary), update)
            assert out["launches"] == [want, want], f"{name}: a hand-off took {out['launches']} launches, the route of this case takes {want}"
    finally:
        s.free()
    return out


def assert_case_specifics(name, update, out):
    """What a case asserts beyond agreement with the model: that the shape it was built for really occurred."""
    case, args = out["case"], out["case"]["args"]
    if case["pre"] or args.n_trees >= 200:
        assert out["nodes"] >= 5, f"{name}: no tree has real depth ({out['nodes']} nodes at most)"
    if name == "z-ragged":
        d = np.diff(np.asarray(args.u))
        assert d.min() == 0 and d.max() == 4 and len(np.unique(d)) >= 3
    if name == "z-fixed-3":
        assert set(np.diff(np.asarray(args.u)).tolist()) == {3}
    if name.startswith("off-") and name != "off-none":
        assert np.ptp(args.offset) > 1e3 * np.ptp(args.y)
    if name.startswith("range-") and update and not args.is_binary:
        r = [float(sc[2]) for sc in out["scales"]]
        lo, hi = (r[1] / r[0], r[2] / r[1]) if name == "range-shrink-grow" else (r[2] / r[1], r[1] / r[0])
        assert lo < 2e-6 and hi > 5e5, (name, r)
        assert max(out["amplification"]) > 1e5 or name == "range-shrink-grow"
    if name.startswith(("n-", "ext-", "off-none")) and update and not args.is_binary and len(args.y) > 3:
        r = [float(sc[2]) for sc in out["scales"]]
        assert 0.2 < r[2] / r[1] < 5.0                        # (a range that stays nearly the same)


def check_create(lib, prefix, binary, report):
    """The create path alone (k_param_mean(fromHost) + k_scale + k_init_residual, trees from the prior, k_assign_leaves(withResidual = 1), the first
    sweep): the state right after create, with a user offset of 1e3 times the response's range."""
    from conftest import StateView, make_sampler
    case = build_case("create-binary" if binary else "create-continuous",
                      dict(n=2 * 4 * handoff_limits()["block"] + 452, offset_type="default", binary=binary, T=5))
    args = case["args"]
    s = make_sampler(lib, prefix, args)
    try:
        sv = StateView(s.get_state())
        _same_bits(sv.get("offset"), np.asarray(args.offset, dtype=np.float64), "BART's offset after create (the user's offset, bart_offset_init = 0)")
        sc = sv.get("scale")
        if binary:
            _same_bits(sc, [-0.5, 0.5, 1.0, 1.0], "the scale of a binary response")
            z = sv.get("latents") + sv.get("offset")
            assert np.all(np.isfinite(z)) and np.array_equal(z > 0, np.asarray(args.y) > 0), "a latent on the wrong side of 0"
        else:
            v = np.asarray(args.y, dtype=np.float64) - sv.get("offset")
            _same_bits(sc[:3], [v.min(), v.max(), v.max() - v.min()], "min / max / range of y - offset after create")
            _ratio(sc[3:4], np.array([args.sigma_init], LD), np.array([4.0 * U * args.sigma_init]), "sigmaData", report)
        assert max(len(nd) for nd, _ in sv.trees) >= 3
        ledger = Ledger(args.n_trees, binary, args.n_thin)
        return audit_state(s, args.x_bart, args, ledger, report, what="after create")
    finally:
        s.free()


def check_parametric_mean_case(lib, prefix, name, report):
    from conftest import make_sampler
    case = build_case(name)
    s = make_sampler(lib, prefix, case["args"])
    try:
        r = s.run(2, True)
        return check_parametric_mean(case["args"], s, r["stan"][:, -1], s.stan_par_names(), report)
    finally:
        s.free()


# ---- free runs under the audit ---------------------------------------------------------------------------------------------------------------------------
def audited_run(lib, prefix, args, warmup, sample, report, setup=None, seed=12345, x_raw=None, teardown=None):
    """create, audit, `warmup` warm-up iterations (scale updates), audit, `sample` sampling iterations, audit.  `setup(s)` runs right after create (tree
    path, test hook, joining a sweep group), `teardown(s)` before it is freed.  Returns (sampler diagnostics for the path assertion, drifts)."""
    from conftest import make_sampler
    s = make_sampler(lib, prefix, args, seed)
    try:
        if setup is not None:
            setup(s)
        ledger = Ledger(args.n_trees, bool(args.is_binary), args.n_thin)
        x = args.x_bart if x_raw is None else x_raw
        drifts = [audit_state(s, x, args, ledger, report, what="after create")]
        sc0 = state_view(s).get("scale")
        s.run(warmup, True)
        ledger.run(warmup, True, args.n_thin)
        drifts.append(audit_state(s, x, args, ledger, report, what="after warm-up"))
        sc1 = state_view(s).get("scale")
        s.disengage_adaptation()
        s.run(sample, False)
        ledger.run(sample, False, args.n_thin)
        drifts.append(audit_state(s, x, args, ledger, report, what="at the end"))
        sc2 = state_view(s).get("scale")
        # (the ledger charges no scale update to a sampling phase: min, max and range must not have moved at all)
        assert np.array_equal(np.asarray(sc1[:3]), np.asarray(sc2[:3])), f"the response scale moved during sampling: {sc1} -> {sc2}"
        report["range across warm-up"] = float(sc0[2] / sc1[2])          # (reported, not asserted: FREE_RUN_AMPLIFICATION is an assumption)
        diag = dict(tree_path=s.get_tree_path(), sweep_stats=s.get_sweep_stats(), sweep_spec=s.get_sweep_spec(), sweep_busy=s.get_sweep_busy(),
                    counters=s.get_counters(), latent_mode=s.get_latent_mode())
        return diag, drifts
    finally:
        if teardown is not None:
            teardown(s)
        s.free()
