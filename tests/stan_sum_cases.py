"""The fixed-point O(N) sums of the Stan block ALONE (k_stan_fused + k_stan_forward + the host's fetch_fused / recentre_scales, and the plain-double
pipeline they fall back to — stan4bart_amd/csrc/dev_hip.hip), one evaluation at a time through the test entry s4b_test_stan_sums: the two references,
the bounds, the constants and the case builders shared by tests/test_gpu_stan_sums.py (libs4b.so on the GPU) and its CPU twin tests/test_stan_sums.py
(the emulated device layer: plain doubles, serial order).  Neither reference shares code with the kernels, the emulation or the oracle.

WHAT IS SUMMED.  e_i = e0_i - x_i' beta - z_i' b (mode -1, "DIRECT") or e_i = response_i - stanOffset_i (modes 0..3; mode 0: e = y); we_i = w_i e_i
(w_i = 1 without weights); ss = sum we_i e_i, (X'e)_k = sum x_ik we_i, (Z'e)_j = sum over the stored entries (i, j) of z we_i.

THE NUMBER FORMAT, as DESIGN.md and the comment above k_stan_fused document it.  grid = min(GRID_CAP, ceil(n / SBLOCK)) workgroups of SBLOCK threads;
observation i belongs to workgroup (i div SBLOCK) mod grid.  Each workgroup forms its partial of ss and of every column of X'e in doubles, multiplies
it by 2^E (E = E_S for ss, E_X for X'e; Z'e: every stored entry on its own, times 2^E_Z), and splits the scaled value v into two limbs,
    hi = rint(v 2^20),  lo = rint((v - hi 2^-20) 2^56)          (round to nearest even; v - hi 2^-20 and both scalings are exact in doubles),
which are added as 64-bit integers (any order: exact).  The host returns (double(sum hi) 2^-20 + double(sum lo) 2^-56) 2^-E.
Beside the sums every workgroup adds, per group g of sums, floor(m 2^-10) + 1 to a MAGNITUDE WORD and takes 4000 + ilogb(m) (m > 0) into the maximum
of an EXPONENT WORD, m being the workgroup's scaled magnitude: |partial of ss| 2^E_S; (sum over rows and ALL K columns of |x we|) 2^E_X; the sum of
|z we| 2^E_Z over its stored entries.  The device raises its FLAG when a scaled partial (ss, X'e) or a scaled entry (Z'e) is not below 2^42 in
absolute value (such an entry of Z'e enters neither limbs nor magnitude; a partial's magnitude is still added) or a magnitude is not below 4e18.
The host rejects the evaluation when the flag is up (1), a magnitude word is 2^32 or more (2), or an exponent word that was written is below
4000 + 4 (4), and repeats it in plain doubles.

EXACT REFERENCE (exact_model).  For data that are integers times powers of two the whole of the above is evaluated in Python integers: e, we, every
product, the workgroup partials, the limbs with their roundings, the integer totals (which must fit 64 bits: "no silent wrap" — a total that does not
fit while the verdict derived from the data says "accepted" fails the comparison), the conversion, the magnitude and exponent words and the verdict.
The model asserts the precondition that makes the doubles on the device exact in ANY order and with or without fused multiply-adds: all terms of a
double sum are multiples of one power of two 2^c and the sum of their absolute values stays below 2^53 2^c (per observation for e; per workgroup for
ss, X'e and the magnitudes; every product's odd part fits 53 bits).  Then an ACCEPTED evaluation must return the model's doubles bit for bit.  Where
every scaled partial is a multiple of 2^-56 the limbs hold the exact sum and the model's value is that sum converted once.  `plain_exact` says
that the same holds over ALL observations: then any plain-double order (the fallback pipeline, the emulation's serial loop) returns the exact sum,
rounded once, bit for bit.

BOUNDED REFERENCE (bounded_model), numpy longdouble, for random data.  u = 2^-53; the comparison allows BOUND_FACTOR = 4 times the bound
(readout_cases.py: the reference's own roundings and the conversion to double).  Ingredients, nothing else:
  (i)   DIRECT: e_i comes out of K + nz_i + 1 rounded operations at most on any one path (a product, the additions after it, the subtraction from e0;
        contraction to FMA only removes roundings), each relative to a partial result no larger than A_i = |e0_i| + sum |x beta| + sum |z b|:
        |de_i| <= (K + nz_i + 1) u A_i.  Mode 0: e = y, de = 0.
  (ii)  we = w e rounds once, we e and x we (and z we) round once more:  |d(we e)| <= 2 |we| de + |w| de^2 + 2 u |we e|,
        |d(x we)| <= |x w| de + 2 u |x we|, likewise z we.
  (iii) ss and X'e, double summation inside one workgroup: `depth` roundings on any one path — the additions of a thread's rows (trips of the
        grid-stride loop), the 6 steps of the wave butterfly, the 3 additions of the four waves — each relative to no more than the workgroup's sum
        of absolute terms; over all workgroups: depth u sum |terms|.
  (iv)  every workgroup partial is rounded to 2^-57 in scaled units: grid 2^-57 2^-E absolute per sum.
  (v)   Z'e: every stored entry is rounded to 2^-57 in scaled units on its own and there is no double summation: nnz_j 2^-57 2^-E_Z for column j.
  (vi)  the host's conversion: two int -> double roundings and one addition.  The low limbs are at most 2^-21 each in scaled units, so with c
        contributions: u (2 |result| + 3 c 2^-21 2^-E).
After a fallback (and where the plain pipeline is the only path) (i)-(iii) apply with the plain pipeline's depth: k_stan_inputs' trips + 6 + 3, then
k_stan_finalize's ceil(grid / 64) + 6 over the partials; Z'e: ceil(CHUNK / BLOCK) + 6 + 3 inside a chunk of k_zt_chunks, then one addition per chunk of
the column.  The emulation adds serially: depth n (nnz_j for a column of Z'e).

THE CHECKS AT THEIR EDGES (edge_cases).  PLANT_A = 127 x 4096, 4095, 90, 9, 3 has sum of squares 2^31 - 1; PLANT_B = 127 x 4096, 4095, 90, 9, 2, 2 has
2^31 - 2; PLANT_C = 128 x 4096 has 2^31.  With y = x = z = the plant (K = 1, one column of Z, coefficients 0) ss, X'e and Z'e and their three
magnitudes are all that number, so one group at a time can be put on a limit by its exponent while the others stay at exponent 0.
  one workgroup, PLANT_A, E = 11: the scaled partial and magnitude are 2^42 - 2^11, the word floor(2^32 - 2) + 1 = 2^32 - 1: the LARGEST magnitude that
  is accepted.  E = 12: ss / X'e: flag (partial >= 2^42) and word; Z'e: word only (its entries are 2^36 at most).
  (The flag's own limit of 2^42 on a partial is therefore never the first to fire: a partial of 2^42 - 2^10 already makes the word 2^32.)
  one workgroup, PLANT_C, E = 11: the partial is 2^42 exactly: flag and word for ss and X'e; Z'e: word only.
  Z'e alone, two rows 1024 and 1 (entries 2^20 and 1), E_Z = 22: one ENTRY is 2^42 exactly: flag only — the entry is left out of the magnitude.
  two workgroups, PLANT_A and PLANT_B, E = 10: words (2^31 - 1 + 1) + (2^31 - 2 + 1) = 2^32 - 1: accepted; PLANT_A twice: 2^32: rejected by
  the word alone (both partials are below 2^42).
  PLANT_A, E = -26: the largest workgroup magnitude is (2^31 - 1) 2^-26, ilogb 4: accepted; E = -27: ilogb 3: rejected by the resolution check alone,
  and the host moves that group's exponent by 22 - 3: to E + 19 (the one adaptation step asserted as a number).

ADAPTATION AS A PROPERTY (adaptation_budget).  The documented rule (comments of fetch_fused / recentre_scales): an evaluation rejected for
resolution alone re-centres every group on its measured exponent at once; an accepted one does the same; after a rejection for range the first
failure is free, every further consecutive one moves each exponent to min(E - 10, 20 - ilogb(|total|)) (E - 10 where the total is 0).  From reset
scales (E = 0) and a stationary input whose workgroup magnitudes are 2^M_g:
  too small (M_g < 4 for a group that is seen, none out of range): evaluation 1 is rejected and re-centred, evaluation 2 is accepted: 2.
  out of range, totals not cancelling (the cases give every product of a sum one sign, so a total is the sum of its workgroup magnitudes; Z'e: the
  largest of three columns is at least a third of it): evaluation 1 is free, evaluation 2 moves E to 20 - ilogb(total) or lower: the total
  then scales below 2^21, every partial and entry with it, and the words stay below 3 (2^11 + grid); if a group has thereby sunk below the
  resolution, evaluation 3 is rejected for resolution and re-centres, evaluation 4 is accepted: at most 4.
  out of range with X'e cancelling to 0 under large magnitudes (scaled_args: every workgroup partial of X'e is exactly 0): the total says nothing
  about the magnitude, only the steps of 10 bits apply to that group: its word falls below 2^32 once grid (2^(M + 1 + E - 10) + 1) < 2^32 (the
  workgroup magnitudes are below 2^(M + 1)), and the partials are 0; with grid <= 2^11 that holds once E <= 20 - M, i.e. after
  ceil((M - 20) / 10) moves, the first of which is made by evaluation 2; one rejection for resolution may follow (the other groups were moved
  down by the same steps): ceil((M - 20) / 10) + 3 evaluations at most, M the binary exponent of the largest workgroup magnitude at E = 0.
Once accepted, the same input is accepted again and the exponents no longer change: an accepted evaluation leaves every group's largest workgroup
magnitude at 2^22, where the next one finds it.  This is asserted as a property of the entry's info (exponents used = exponents left), as is the
verdict of every evaluation on the way: it must be the verdict the data imply under the exponents of that launch.  Beyond the clamp of +-900 no
exponent brings ss into range (BEYOND_CLAMP): every evaluation falls back, and every result is still the exact sum.
"""
import math
import os
import re

import numpy as np

from handoff_cases import geometry as plain_geometry
from large_cases import stan_kernel_branch, stan_shape_case, stan_shape_of
from readout_cases import BOUND_FACTOR, U, bound_ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_HIP = os.path.join(ROOT, "stan4bart_amd", "csrc", "dev_hip.hip")
LD = np.longdouble
REJECT_FLAG, REJECT_WORD, REJECT_TINY = 1, 2, 4


# ---- the constants, read from the source -------------------------------------------------------------------------------------------------------------
def limits(src_path=DEV_HIP):
    """The constants of the fixed-point sums, READ from dev_hip.hip; the statements this module restates are asserted to still be there, so that a
    moved threshold moves the expectation (or fails here) instead of quietly retargeting a case."""
    src = open(src_path).read()

    def const(name):
        return int(re.search(r"constexpr int " + name + r" = (\d+);", src).group(1))
    L = dict(sblock=const("SBLOCK"), copies=const("S_COPIES"), qmax=const("S_QMAX"), zmax=const("S_ZMAX"), inline=const("S_PAR_INLINE"), block=const("BLOCK"))
    m = re.search(r"constexpr double S_FX_LIMIT = (\d+)\.0;", src)
    assert m, "S_FX_LIMIT is no longer a literal"
    L["fx_limit"] = int(m.group(1))
    assert L["fx_limit"] & (L["fx_limit"] - 1) == 0
    m = re.search(r"const int grid = \(int\)std::min<int64_t>\((\d+), std::max<int64_t>\(1, \(n_ \+ SBLOCK - 1\) / SBLOCK\)\);", src)
    assert m, "the grid of k_stan_fused is no longer min(cap, ceil(n / SBLOCK))"
    L["grid_cap"] = int(m.group(1))
    m = re.search(r"for \(int g = 0; g < 3; \+\+g\) if \(mag\[g\] >= \(1ull << (\d+)\)\) why \|= 2;", src)
    assert m, "the magnitude-word check changed"
    L["word_bits"] = int(m.group(1))
    m = re.search(r"if \(seen\[g\] && ex\[g\] < (\d+)\) why \|= 4;", src)
    assert m, "the resolution check changed"
    L["ex_min"] = int(m.group(1))
    m = re.findall(r"fxExp_\[g\] = std::max\(-(\d+), std::min\((\d+), fxExp_\[g\] \+ \((\d+) - ex\[g\]\)\)\);", src)
    assert len(m) == 2 and m[0] == m[1] and m[0][0] == m[0][1], "the re-centring of the scales changed"
    L["clamp"], L["target"] = int(m[0][0]), int(m[0][2])
    m = re.search(r"int want = fxExp_\[g\] - (\d+);\s*if \(tot\[g\] > 0\.0\) want = std::min\(want, (\d+) - std::ilogb\(tot\[g\]\)\);", src)
    assert m, "recentre_scales changed"
    L["step"], L["total_target"] = int(m.group(1)), int(m.group(2))
    for stmt in ("const double SH = 1048576.0, SL = 72057594037927936.0;   // 2^20, 2^56",
                 "const double h = rint(v * SH);",
                 "FxLimbs r; r.hi = (long long)h; r.lo = (long long)rint((v - h / SH) * SL);",
                 "unsigned long long* mine = f.acc + ((size_t)f.parity * S_COPIES + (blockIdx.x % S_COPIES)) * W;",
                 "if (!(fabs(c) < S_FX_LIMIT)) { bad = 1; return; }",
                 "if (!(fabs(v) < S_FX_LIMIT)) bad = 1;",
                 "if (!(m < 4.0e18)) bad = 1;",
                 "atomicAdd(mine + 2 * (size_t)M + g, (unsigned long long)(m * 0.0009765625) + 1ull);",
                 "if (m > 0.0) atomicMax(mine + 2 * (size_t)M + 3 + g, (unsigned long long)(ilogb(m) + 4000));",
                 "m = g == 0 ? fabs(m) * sS : (g == 1 ? m * sX : m);",
                 "return ((double)hi / 1048576.0 + (double)lo / 72057594037927936.0) * inv[g];",
                 "seen[g] = m != 0; ex[g] = (int)m - 4000;",
                 "const int64_t stride = (int64_t)gridDim.x * SBLOCK;",
                 "const int CHUNK = 4096;",
                 "void reset_fused_scales() { fxExp_[0] = fxExp_[1] = fxExp_[2] = 0; fxLastBad_ = -2; fxTinyFail_ = false; }"):
        assert stmt in src, stmt
    L["chunk"] = 4096
    return L


def fused_grid(n, L=None):
    L = L or limits()
    return min(L["grid_cap"], max(1, -(-n // L["sblock"])))


# ---- the data of a case ------------------------------------------------------------------------------------------------------------------------------
class Data:
    """What create was given, as float64 arrays: y, X [n, K], the CSR triplet of Z (w, v, u), the weights (or None)."""

    def __init__(self, args):
        self.n = len(args.y)
        self.y = np.asarray(args.y, dtype=np.float64)
        self.X = np.asarray(args.X, dtype=np.float64).reshape(self.n, -1) if args.X is not None else np.zeros((self.n, 0))
        self.K = self.X.shape[1]
        self.q = int(sum(int(a) * int(c) for a, c in zip(args.p, args.l)))
        self.w = np.asarray(args.w, dtype=np.float64)
        self.v = np.asarray(args.v, dtype=np.int64)
        self.u = np.asarray(args.u, dtype=np.int64)
        self.rows = np.repeat(np.arange(self.n), np.diff(self.u)) if self.q else np.zeros(0, np.int64)
        self.wts = None if args.weights is None else np.asarray(args.weights, dtype=np.float64)
        self.nz = np.diff(self.u) if self.q else np.zeros(self.n, np.int64)


def dyadic(args, seed, y_bits=4, x_bits=3, z_bits=2, empty_rows=False):
    """Overwrite the numbers of a stan_shape_case with small integers times powers of two, keeping its shape (K, the pattern of Z, weights or
    not): y in +-2^y_bits / 4, X in +-2^x_bits / 2, the stored values of Z in +-2^z_bits without 0, weights in {1/4, 1/2, 1, 2, 4}.  `empty_rows`: a fifth
    of the rows lose every stored entry of Z (rows with no stored entry; the row pointers become general)."""
    g = np.random.default_rng(9100000 + seed)
    n = len(args.y)
    y = g.integers(-(1 << y_bits), (1 << y_bits) + 1, n).astype(np.float64) / 4.0
    if n > 1 and np.ptp(y) == 0:
        y[0] += 1.0
    if n == 1:
        y[:] = 2.75
    args.y = y
    if args.X is not None and np.asarray(args.X).size:
        K = np.asarray(args.X).reshape(n, -1).shape[1]
        args.X = np.asfortranarray(g.integers(-(1 << x_bits), (1 << x_bits) + 1, (n, K)).astype(np.float64) / 2.0)
    nnz = len(np.asarray(args.w))
    if nnz:
        wv = g.integers(1, (1 << z_bits) + 1, nnz).astype(np.float64) * g.choice([-1.0, 1.0], nnz)
        args.w = wv
        if empty_rows:
            u = np.asarray(args.u, dtype=np.int64)
            rows = np.repeat(np.arange(n), np.diff(u))
            drop = g.random(n) < 0.2
            drop[0] = False
            drop[n - 1] = True
            keep = ~drop[rows]
            cnt = np.bincount(rows[keep], minlength=n)
            args.u = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
            args.w = wv[keep].copy()
            args.v = np.asarray(args.v)[keep].copy()
    if args.weights is not None:
        args.weights = g.choice([0.25, 0.5, 1.0, 2.0, 4.0], n)
    return args


def small_coefficients(K, q, seed):
    """beta, b: small integers over 2 (exact products with dyadic() data)."""
    g = np.random.default_rng(9200000 + seed)
    return g.integers(-3, 4, K).astype(np.float64) / 2.0, g.integers(-3, 4, q).astype(np.float64) / 2.0


# ---- exact arithmetic on doubles: (Python integers, one binary exponent) -------------------------------------------------------------------------------
def _ints(a):
    """Object array of Python integers I and an exponent c with a = I 2^c, exactly."""
    a = np.asarray(a, dtype=np.float64)
    assert np.all(np.isfinite(a))
    m, e = np.frexp(a)
    mi = (m * 9007199254740992.0).astype(np.int64)          # m 2^53: an integer
    e = e.astype(np.int64) - 53
    nzm = mi != 0
    if not nzm.any():
        return np.zeros(a.shape, dtype=object), 0
    tz = np.zeros(a.shape, np.int64)                            # trailing zeros of every mantissa: the element is odd 2^(e + tz)
    low = mi & -mi
    tz[nzm] = np.round(np.log2(low[nzm].astype(np.float64))).astype(np.int64)
    c = int((e + tz)[nzm].min())
    out = np.array([(int(x) >> int(t)) << int(k + t - c) if x else 0 for x, k, t in zip(mi.ravel().tolist(), e.ravel().tolist(), tz.ravel().tolist())],
                   dtype=object).reshape(a.shape)
    return out, c


def _align(a, ca, b, cb):
    c = min(ca, cb)
    return a * (1 << (ca - c)) if ca > c else a, b * (1 << (cb - c)) if cb > c else b, c


def _rne_scale(p, k):
    """round-half-even of p 2^k, p a Python integer."""
    if k >= 0:
        return p << k
    d = 1 << (-k)
    fl, r = p >> (-k), p & (d - 1)
    half = d >> 1
    if r > half or (r == half and (fl & 1)):
        fl += 1
    return fl


def _odd_bits(x):
    x = abs(int(x))
    return 0 if x == 0 else (x >> ((x & -x).bit_length() - 1)).bit_length()


def _ilogb(p, c):
    """ilogb of p 2^c, p a positive Python integer."""
    return p.bit_length() - 1 + c


def _to_float(p, c):
    """p 2^c rounded once to a double."""
    from fractions import Fraction
    return float(Fraction(p) * (Fraction(2) ** c))


def _group_sum(values, index, size):
    out = np.zeros(size, dtype=object)
    np.add.at(out, index, values)
    return out


def _sum_is_exact(abs_terms, index, size):
    """Per group of `index`: are all terms multiples of one power of two 2^c with the sum of their absolute values below 2^53 2^c?  Then a double
    summation of that group is exact in any order.  Returns (the sums of absolute values, the bitwise OR of the absolute values, verdict)."""
    tot, orv = np.zeros(size, dtype=object), np.zeros(size, dtype=object)
    np.add.at(tot, index, abs_terms)
    np.bitwise_or.at(orv, index, abs_terms)
    ok = all(int(t) == 0 or (int(t) // (int(o) & -int(o))).bit_length() <= 53 for t, o in zip(tot.tolist(), orv.tolist()))
    return tot, orv, ok


def _limbs(p, s):
    """The two limbs of the scaled value p 2^(s - 56): hi in units of 2^-20, lo in units of 2^-56."""
    if s - 36 >= 0:
        return p << (s - 36), 0
    hi = _rne_scale(p, s - 36)
    return hi, _rne_scale(p - (hi << (36 - s)), s)


def exact_model(data, mode, beta, b, exps, L=None):
    """The whole evaluation in integers (module docstring).  mode -1: e = e0 - X beta - Z b with e0 = y (the sampler's last evaluation of the other kind
    was mode 0); mode 0: e = y.  Returns dict(fused = the doubles an accepted evaluation returns, total = the exact sums rounded once, reject, flag,
    mag, exw, grid, wrapped, plain_exact, multiples = every scaled partial is a multiple of 2^-56, top = per group the binary exponent of the largest scaled
    workgroup magnitude, None where nothing but zeros went in)."""
    L = L or limits()
    n, K, q = data.n, data.K, data.q
    grid = fused_grid(n, L)
    wg = (np.arange(n) // L["sblock"]) % grid
    # -- e and we
    e, ce = _ints(data.y)
    mag_e = np.abs(e)
    if mode < 0:
        for k in range(K):
            xi, cx = _ints(data.X[:, k])
            bi, cb = _ints(np.array([beta[k]]))
            t, ct = xi * bi[0], cx + cb
            e, t, ce2 = _align(e, ce, t, ct)
            mag_e = mag_e * (1 << (ce - ce2)) + np.abs(t)
            e, ce = e - t, ce2
        if q and len(data.w):
            wi, cw = _ints(data.w)
            bi, cb = _ints(np.asarray(b, dtype=np.float64))
            t = _group_sum(wi * bi[data.v], data.rows, n)
            ta = _group_sum(np.abs(wi * bi[data.v]), data.rows, n)
            ct = cw + cb
            e, t, ce2 = _align(e, ce, t, ct)
            ta = ta * (1 << (ct - ce2))
            mag_e = mag_e * (1 << (ce - ce2)) + ta
            e, ce = e - t, ce2
    else:
        assert mode == 0, "the exact model knows e = y and e = y - X beta - Z b"
    # (every term of e is a multiple of 2^ce; |partial results| <= mag_e)
    assert all(int(m).bit_length() <= 53 for m in mag_e.tolist()), "e is not exact in doubles for this data"
    if data.wts is not None:
        ti, cwt = _ints(data.wts)
        we, cwe = ti * e, cwt + ce
    else:
        we, cwe = e, ce
    assert all(_odd_bits(x) <= 53 for x in we.tolist()), "w e is not exact in doubles for this data"
    M = 1 + K + q
    hi_tot, lo_tot, exact_tot = [0] * M, [0] * M, [None] * M
    flag = False
    multiples = True
    plain_exact = True
    mag_exact = True
    mags = [np.zeros(grid, dtype=object) for _ in range(3)]           # scaled magnitudes per workgroup, with the exponents below
    mag_c = [0, 0, 0]

    def partial_group(terms, ct, E, k, g, mag_terms=None):
        nonlocal flag, multiples, plain_exact
        part = _group_sum(terms, wg, grid)
        pabs, por, ok = _sum_is_exact(np.abs(terms), wg, grid)
        assert ok, "a workgroup partial is not exact in doubles for this data"
        plain_exact = plain_exact and _sum_is_exact(np.abs(terms), np.zeros(n, np.int64), 1)[2]
        s = ct + E + 56
        multiples = multiples and s >= 0
        for p in part.tolist():
            if abs(p) << max(s - 56, 0) >= L["fx_limit"] << max(56 - s, 0):          # |p| 2^(s - 56) >= 2^42
                flag = True
                continue
            hi, lo = _limbs(p, s)
            hi_tot[k] += hi
            lo_tot[k] += lo
        exact_tot[k] = (int(part.sum()), ct)
        return part, pabs, por

    # -- ss
    t0 = we * e
    part0, _, _ = partial_group(t0, cwe + ce, exps[0], 0, 0)
    mags[0], mag_c[0] = np.abs(part0), cwe + ce + exps[0]
    # -- X'e
    mx, mor = np.zeros(grid, dtype=object), np.zeros(grid, dtype=object)
    cmx = None
    for k in range(K):
        xi, cx = _ints(data.X[:, k])
        t = xi * we
        assert all(_odd_bits(x) <= 53 for x in t.tolist())
        _, pabs, por = partial_group(t, cx + cwe, exps[1], 1 + k, 1)
        if cmx is None:
            mx, mor, cmx = pabs, por, cx + cwe
        else:
            sh_old, sh_new = cmx - min(cmx, cx + cwe), cx + cwe - min(cmx, cx + cwe)
            mx, mor, cmx = mx * (1 << sh_old) + pabs * (1 << sh_new), (mor * (1 << sh_old)) | (por * (1 << sh_new)), min(cmx, cx + cwe)
    if K:
        assert all(int(t) == 0 or (int(t) // (int(o) & -int(o))).bit_length() <= 53 for t, o in zip(mx.tolist(), mor.tolist())), \
            "the magnitude of X'e is not exact in doubles for this data"
        mags[1], mag_c[1] = mx, cmx + exps[1]
    # -- Z'e: every stored entry on its own
    if q:
        for j in range(q):
            exact_tot[1 + K + j] = (0, 0)
    if q and len(data.w):
        wi, cw = _ints(data.w)
        c = wi * we[data.rows]
        cc = cw + cwe
        assert all(_odd_bits(x) <= 53 for x in c.tolist())
        s = cc + exps[2] + 56
        multiples = multiples and s >= 0
        wge = wg[data.rows]
        mz, mzor = np.zeros(grid, dtype=object), np.zeros(grid, dtype=object)
        col_abs, col_or = [0] * q, [0] * q
        col_sum = [0] * q
        for val, col, g_ in zip(c.tolist(), data.v.tolist(), wge.tolist()):
            col_sum[col] += val
            col_abs[col] += abs(val)
            col_or[col] |= abs(val)
            if abs(val) << max(s - 56, 0) >= L["fx_limit"] << max(56 - s, 0):
                flag = True
                continue
            mz[g_] += abs(val)
            mzor[g_] |= abs(val)
            hi, lo = _limbs(val, s)
            hi_tot[1 + K + col] += hi
            lo_tot[1 + K + col] += lo
        for j in range(q):
            exact_tot[1 + K + j] = (col_sum[j], cc)
            plain_exact = plain_exact and (col_abs[j] == 0 or (col_abs[j] // (col_or[j] & -col_or[j])).bit_length() <= 53)
        # (a magnitude that is not exact in doubles — 2^21 and 2^-50 in one workgroup — is a rounded sum on the device: its word is then not compared)
        mag_exact = all(int(t) == 0 or (int(t) // (int(o) & -int(o))).bit_length() <= 53 for t, o in zip(mz.tolist(), mzor.tolist()))
        mags[2], mag_c[2] = mz, cc + exps[2]
    # -- the words and the verdict
    word, exw, top = [0, 0, 0], [0, 0, 0], [None, None, None]
    for g in range(3):
        for m in mags[g].tolist():
            m = int(m)
            c = mag_c[g]
            if m > 0:
                top[g] = max(_ilogb(m, c), -10 ** 9 if top[g] is None else top[g])
            big = (m << c if c >= 0 else m >> (-c)) >= 4 * 10 ** 18          # (floor of the magnitude against an integer limit)
            if big:
                flag = True
                continue
            word[g] += (m << (c - 10) if c >= 10 else m >> (10 - c)) + 1
            if m > 0:
                exw[g] = max(exw[g], _ilogb(m, c) + 4000)
    reject = (REJECT_FLAG if flag else 0)
    reject |= REJECT_WORD if any(w >= 1 << L["word_bits"] for w in word) else 0
    reject |= REJECT_TINY if any(x and x - 4000 < L["ex_min"] for x in exw) else 0
    wrapped = any(not -(1 << 63) <= x < (1 << 63) for x in hi_tot + lo_tot)
    fused = np.zeros(M)
    total = np.zeros(M)
    for k in range(M):
        E = exps[0] if k == 0 else exps[1] if k <= K else exps[2]
        hi = (hi_tot[k] + (1 << 63)) % (1 << 64) - (1 << 63)
        lo = (lo_tot[k] + (1 << 63)) % (1 << 64) - (1 << 63)
        fused[k] = (float(hi) / 1048576.0 + float(lo) / 72057594037927936.0) * math.ldexp(1.0, -E)
        total[k] = _to_float(*exact_tot[k])
    return dict(fused=fused, total=total, reject=reject, flag=flag, mag=tuple(word), exw=tuple(exw), grid=grid, wrapped=wrapped,
                plain_exact=plain_exact, multiples=multiples, top=tuple(top), mag_exact=mag_exact)


# ---- the bounded reference -----------------------------------------------------------------------------------------------------------------------------
def depths(data, path, L=None):
    """Roundings on any one path of the double summations (module docstring (iii)): dict(ssx = for ss and the columns of X'e, z = per column of Z'e).
    path: "fused", "plain" (the fallback pipeline on the device) or "serial" (the emulation)."""
    L = L or limits()
    n, q = data.n, data.q
    nnz_col = np.bincount(data.v, minlength=q) if q else np.zeros(0, np.int64)
    if path == "fused":
        grid = fused_grid(n, L)
        return dict(ssx=-(-n // (grid * L["sblock"])) + 6 + 3, z=np.zeros(q))
    if path == "plain":
        gm = plain_geometry(n)
        per_chunk = -(-L["chunk"] // gm["block"]) + 6 + 3
        return dict(ssx=gm["trips"] + 6 + 3 + -(-gm["grid"] // 64) + 6, z=per_chunk + -(-nnz_col // L["chunk"]))
    assert path == "serial"
    return dict(ssx=n, z=nnz_col.astype(np.float64))


def bounded_model(data, e0, beta, b, exps, path, de0=None, L=None):
    """(reference [1 + K + q] in long double, bound [1 + K + q]) for e = e0 - X beta - Z b (beta = b = None: e = e0), module docstring (i)-(vi).
    e0: the doubles on the device (y after a mode-0 evaluation), or a long-double model of them with its own error bound de0 per observation."""
    L = L or limits()
    n, K, q = data.n, data.K, data.q
    e = np.asarray(e0).astype(LD)
    A = np.abs(e)
    if beta is not None:
        for k in range(K):
            t = data.X[:, k].astype(LD) * LD(beta[k])
            e = e - t
            A = A + np.abs(t)
        if q and len(data.w):
            t = data.w.astype(LD) * np.asarray(b, dtype=np.float64)[data.v].astype(LD)
            zs, za = np.zeros(n, LD), np.zeros(n, LD)
            np.add.at(zs, data.rows, t)
            np.add.at(za, data.rows, np.abs(t))
            e = e - zs
            A = A + za
        de = (K + data.nz + 1) * LD(U) * A
    else:
        de = np.zeros(n, LD)
    if de0 is not None:
        de = de + np.asarray(de0).astype(LD)
    w = np.ones(n, LD) if data.wts is None else data.wts.astype(LD)
    we = w * e
    d = depths(data, path, L)
    grid = fused_grid(n, L)
    M = 1 + K + q
    ref, bound = np.zeros(M, LD), np.zeros(M, LD)

    def fixed_point(result, contributions, E):
        sc = LD(2.0) ** (-E)
        return contributions * LD(2.0) ** -57 * sc + LD(U) * (2 * abs(result) + 3 * contributions * LD(2.0) ** -21 * sc)
    t = we * e
    ref[0] = t.sum()
    bound[0] = (2 * np.abs(we) * de + np.abs(w) * de * de + 2 * LD(U) * np.abs(t)).sum() + d["ssx"] * LD(U) * np.abs(t).sum()
    if path == "fused":
        bound[0] += fixed_point(ref[0], grid, exps[0])
    for k in range(K):
        x = data.X[:, k].astype(LD)
        t = x * we
        ref[1 + k] = t.sum()
        bound[1 + k] = (np.abs(x * w) * de + 2 * LD(U) * np.abs(t)).sum() + d["ssx"] * LD(U) * np.abs(t).sum()
        if path == "fused":
            bound[1 + k] += fixed_point(ref[1 + k], grid, exps[1])
    if q:
        if len(data.w):
            z = data.w.astype(LD)
            t = z * we[data.rows]
            term = np.abs(z * w[data.rows]) * de[data.rows] + 2 * LD(U) * np.abs(t)
            zs, zb, za = np.zeros(q, LD), np.zeros(q, LD), np.zeros(q, LD)
            np.add.at(zs, data.v, t)
            np.add.at(zb, data.v, term)
            np.add.at(za, data.v, np.abs(t))
            nnz_col = np.bincount(data.v, minlength=q)
            ref[1 + K:] = zs
            bound[1 + K:] = zb + np.asarray(d["z"], dtype=np.float64) * LD(U) * za
            if path == "fused":
                for j in range(q):
                    bound[1 + K + j] += fixed_point(zs[j], int(nnz_col[j]), exps[2])
    return ref, bound.astype(np.float64)


def check_bounded(sums, ref, bound, what, report):
    r = bound_ratio(sums, ref, bound)
    report[what] = max(report.get(what, 0.0), r)
    assert r <= BOUND_FACTOR, f"{what}: |sums - model| is {r:.3g} x the derived bound (allowed: {BOUND_FACTOR:g})"
    return r


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    bad = np.flatnonzero(a.view(np.uint64) != b.view(np.uint64))
    assert bad.size == 0, f"{what}: not bit-identical at {bad[:8].tolist()}: {a[bad[:4]].tolist()} against {b[bad[:4]].tolist()}"


# ---- case builders ---------------------------------------------------------------------------------------------------------------------------------------
def shape_case(n, K, terms, seed, weights=False, ragged=False, empty_rows=False, exact=True, no_entries=False):
    """Sampler arguments of a chosen parametric shape (large_cases.stan_shape_case: hmc_mode 1, two trees, plain starting values), with dyadic()
    numbers when `exact`.  `no_entries`: Z keeps its q columns and loses every stored entry (every row has 0 of them)."""
    args = stan_shape_case(n, K, terms, 7000 + seed, 1, weights=weights, ragged=ragged, iters=(2, 4), trees=2, plain_init=True)
    if exact:
        dyadic(args, seed, empty_rows=empty_rows)
    if no_entries:
        args.w, args.v, args.u = np.zeros(0), np.zeros(0, np.int32), np.zeros(n + 1, np.int32)
    if not args.sigma_init > 0.0:                               # (a least-squares fit of one row is saturated; where the chain starts is not the subject)
        args.sigma_init = 1.0
    if n == 1:                                                  # (the autoscaled priors divide by the standard deviation of one number)
        args.prior_scale = np.ones(K)
        args.prior_scale_for_aux = 1.0
    return args


def geometry_cases(L=None):
    """name -> keywords of shape_case: the launch geometry and every branch of k_stan_fused a shape selects (module docstring of the GPU test)."""
    L = L or limits()
    B, C, cap = L["sblock"], L["copies"], L["grid_cap"]
    G = {}
    G["n1"] = dict(n=1, K=1, terms=[(1, 0)])
    for n in (B // 4 - 1, B // 4, B - 1, B, B + 1):
        G["n%d" % n] = dict(n=n, K=2, terms=[(3, 1)], weights=n % 2 == 0)
    G["n-33-workgroups"] = dict(n=C * B + 1, K=2, terms=[(5, 0)])                       # copy 0 is used twice
    G["n-64-workgroups"] = dict(n=2 * C * B, K=1, terms=[(5, 1)], weights=True)         # every copy is used twice
    G["n-grid-cap"] = dict(n=cap * B + B + 1, K=2, terms=[(4, 0)])                      # the cap, the grid-stride loop, a ragged second pass
    for K in (1, 2, 3, 4, 5, 8, 9, 16):                                                 # first and last K of KMAX 2 / 4 / 8 / 16
        G["K%d" % K] = dict(n=300, K=K, terms=[(4, 0)], weights=K in (3, 8, 16))
    G["K0"] = dict(n=300, K=0, terms=[(6, 1)])
    G["q0"] = dict(n=300, K=3, terms=[])
    G["z0"] = dict(n=300, K=2, terms=[(4, 0)], no_entries=True)
    G["z3"] = dict(n=300, K=2, terms=[(5, 1), (3, 0)])
    G["z4"] = dict(n=300, K=2, terms=[(5, 1), (3, 1)], weights=True)
    G["z5"] = dict(n=400, K=2, terms=[(6, 2), (4, 1)])
    G["z-ragged"] = dict(n=400, K=5, terms=[(5, 1), (3, 1)], ragged=True)
    G["z-empty-rows"] = dict(n=400, K=2, terms=[(5, 1), (3, 1)], empty_rows=True, weights=True)
    G["q512"] = dict(n=1100, K=2, terms=[(512, 0)])
    G["q513"] = dict(n=1100, K=2, terms=[(513, 0)], weights=True)
    G["inline-64"] = dict(n=500, K=12, terms=[(52, 0)])
    G["params-65"] = dict(n=500, K=12, terms=[(53, 0)], weights=True)
    return G


def expected_branch(spec, args, L=None):
    """stan_kernel_branch of the case plus its grid."""
    K, q, nz = stan_shape_of(args)
    br = stan_kernel_branch(K, q, nz)
    br["grid"] = fused_grid(len(args.y), L)
    return br


PLANT_A = [4096] * 127 + [4095, 90, 9, 3]                    # sum of squares 2^31 - 1
PLANT_B = [4096] * 127 + [4095, 90, 9, 2, 2]                 # 2^31 - 2
PLANT_C = [4096] * 128                                       # 2^31
assert sum(v * v for v in PLANT_A) == 2 ** 31 - 1 and sum(v * v for v in PLANT_B) == 2 ** 31 - 2 and sum(v * v for v in PLANT_C) == 2 ** 31


def planted_case(workgroups, seed=0, L=None):
    """K = 1, one column of Z; y = x = the stored values of Z = the plants, one plant at the start of each workgroup (the rest of a workgroup: zeros)."""
    L = L or limits()
    B = L["sblock"]
    n = B * (len(workgroups) - 1) + len(workgroups[-1])
    v = np.zeros(n)
    for g, plant in enumerate(workgroups):
        assert len(plant) <= B
        v[g * B:g * B + len(plant)] = plant
    args = stan_shape_case(n, 1, [(1, 0)], 7900 + seed, 1, iters=(2, 4), trees=2, plain_init=True)
    args.y = v.copy()
    args.X = np.asfortranarray(v.reshape(n, 1).copy())
    args.w = v.copy()
    return args


def vector_case(values, x=None, z=None, K=1, seed=0):
    """K = 1 (or 0), one column of Z; y = `values`, x and the stored values of Z as given (default: ones)."""
    values = np.asarray(values, dtype=np.float64)
    n = len(values)
    args = stan_shape_case(n, K, [(1, 0)], 7950 + seed, 1, iters=(2, 4), trees=2, plain_init=True)
    args.y = values.copy()
    if K:
        args.X = np.asfortranarray((np.ones(n) if x is None else np.asarray(x, dtype=np.float64)).reshape(n, 1).copy())
    args.w = np.ones(n) if z is None else np.asarray(z, dtype=np.float64).copy()
    args.bart_offset_init, args.sigma_init = np.zeros(n), 1.0          # (where the chain starts is not the subject; a fit of two rows is saturated)
    return args


def adaptation_budget(M_top, out_of_range, cancelling, L=None):
    """Evaluations allowed before the first accepted one, from reset scales (module docstring, ADAPTATION AS A PROPERTY)."""
    L = L or limits()
    if not out_of_range:
        return 2
    if not cancelling:
        return 4
    return -(-(M_top - L["total_target"]) // L["step"]) + 3


# ---- drivers shared by the two test files ------------------------------------------------------------------------------------------------------------
def centred_exps(data, mode, beta, b, L=None):
    """Exponents that put the largest workgroup magnitude of every group at 2^target — from the model at exponents 0, not from the product."""
    L = L or limits()
    m = exact_model(data, mode, beta, b, (0, 0, 0), L)
    return tuple(L["target"] - x if x is not None else 0 for x in m["top"])


def check_exact(impl, fused_shape, sums, info, model, exps, what):
    """One evaluation of exact data against exact_model: on the device the verdict, the words and the grid equal the model's, an accepted result equals
    the model's doubles bit for bit; a rejected one, a shape without the fixed-point path and the emulation equal the exact sums rounded once (the
    data must then be exact in any plain-double order).  Returns the path taken: "fused" or "plain"."""
    if impl == "s4b" and fused_shape:
        assert info["fused"], f"{what}: the entry reports a shape without the fixed-point path"
        assert info["grid"] == model["grid"], f"{what}: {info['grid']} workgroups, the geometry of this n has {model['grid']}"
        assert info["exp_used"] == tuple(exps), f"{what}: launched with exponents {info['exp_used']}, expected {tuple(exps)}"
        assert info["mag"] == model["mag"] or not model["mag_exact"], f"{what}: magnitude words {info['mag']}, derived from the data {model['mag']}"
        assert info["exw"] == model["exw"], f"{what}: exponent words {info['exw']}, derived from the data {model['exw']}"
        assert info["reject"] == model["reject"], f"{what}: rejected by {info['reject']}, derived from the data {model['reject']}"
        assert info["accepted"] == (model["reject"] == 0)
        if info["accepted"]:
            assert not model["wrapped"], f"{what}: a limb total leaves 64 bits although every check passed"
            same_bits(sums, model["fused"], what + " (accepted)")
            return "fused"
    else:
        assert not info["fused"] and not info["accepted"] and info["reject"] == 0 and info["exp_used"] == (0, 0, 0) and info["exp_after"] == (0, 0, 0), what
    assert model["plain_exact"], f"{what}: the data of this case are not exact in every plain-double order"
    same_bits(sums, model["total"], what + " (plain doubles)")
    return "plain"


def open_case(lib, prefix, args):
    from conftest import make_sampler
    return make_sampler(lib, prefix, args), Data(args), prefix.rstrip("_")


def run_geometry_case(lib, prefix, name, L=None):
    """Case a: mode 0 and then DIRECT with small coefficients, both with centred exponents; every result exact, on the fused path where there is one."""
    import zlib
    L = L or limits()
    spec = geometry_cases(L)[name]
    seed = zlib.crc32(name.encode()) % 1000
    args = shape_case(seed=seed, **spec)
    br = expected_branch(spec, args, L)
    s, data, impl = open_case(lib, prefix, args)
    out = dict(branch=br, paths=[], info=[])
    try:
        beta, b = small_coefficients(data.K, data.q, seed)
        for mode, bt, bb in ((0, None, None), (-1, beta, b)):
            exps = centred_exps(data, mode, bt, bb, L)
            model = exact_model(data, mode, bt, bb, exps, L)
            assert model["reject"] == 0 and model["multiples"], f"{name}: the case is not in range at centred exponents"
            same_bits(model["fused"], model["total"], f"{name}: the model's own two conversions")
            sums, info = s.test_stan_sums(mode, bt, bb, set_exp=exps)
            out["paths"].append(check_exact(impl, br["fused"], sums, info, model, exps, f"{name} mode {mode}"))
            out["info"].append(info)
            assert np.abs(sums).max() > 0
    finally:
        s.free()
    return out


def cancellation_args(order, t, L=None):
    """Case b: K = 1, one column of Z, three workgroups; e = 1 at five rows and 0 elsewhere.  The X column holds (2^21, -2^21, t) in the order `order` in
    three different workgroups; the Z column holds the same three values in two waves of workgroup 0 and in workgroup 1."""
    L = L or limits()
    B = L["sblock"]
    n = 3 * B
    vals = [[2.0 ** 21, -2.0 ** 21, float(t)][k] for k in order]
    rows_x, rows_z = (0, B, 2 * B), (0, 64 + 5, B + 130)
    y, x, z = np.zeros(n), np.zeros(n), np.zeros(n)
    y[list(set(rows_x + rows_z))] = 1.0
    x[list(rows_x)] = vals
    z[list(rows_z)] = vals
    return vector_case(y, x=x, z=z, seed=sum(order)), len(set(rows_x + rows_z))


def run_cancellation(lib, prefix, order, t, L=None):
    L = L or limits()
    args, ones = cancellation_args(order, t, L)
    s, data, impl = open_case(lib, prefix, args)
    try:
        exps = (10, 0, 0)
        model = exact_model(data, 0, None, None, exps, L)
        assert model["reject"] == 0 and not model["wrapped"]
        assert model["fused"].tolist() == [float(ones), float(t), float(t)], model["fused"]
        sums, info = s.test_stan_sums(0, set_exp=exps)
        if impl != "s4b" and not model["plain_exact"]:
            # plain doubles keep 2^-50 beside 2^21 only in a lucky order (that is what the integer limbs are for): the emulation's serial sums are
            # held to the serial bound, the model's own claim — the exact total — is asserted above
            ref, bound = bounded_model(data, data.y, None, None, exps, "serial", L=L)
            check_bounded(sums, ref, bound, "cancellation, serial", {})
            return "plain"
        path = check_exact(impl, True, sums, info, model, exps, f"cancellation {order} t = {t}")
        assert sums.tolist() == [float(ones), float(t), float(t)]
        assert np.signbit(sums[1]) == np.signbit(float(t)) or t == 0
        return path
    finally:
        s.free()


def run_hygiene(lib, prefix, L=None):
    """Case c: the same evaluation four times (both accumulator parities twice); accepted -> rejected for range -> accepted -> accepted and the same
    with a rejection for resolution; every accepted result is the exact model's, every verdict the one derived from the data."""
    L = L or limits()
    args = shape_case(n=2 * L["copies"] * L["sblock"] + 77, K=3, terms=[(5, 1)], seed=41, weights=True)
    s, data, impl = open_case(lib, prefix, args)
    paths = []
    try:
        beta, b = small_coefficients(data.K, data.q, 41)
        s.test_stan_sums(0, set_exp=(0, 0, 0))                       # (e0 = y for the DIRECT evaluations below)
        good = centred_exps(data, -1, beta, b, L)
        high = tuple(e + 40 for e in good)                           # largest workgroup magnitude 2^62: out of range
        low = tuple(e - 30 for e in good)                            # 2^-8: below the resolution
        runs = [good] * 4 + [good, high, good, good] + [good, low, good, good] + [high, low, high, good, good]
        first = None
        models = {exps: exact_model(data, -1, beta, b, exps, L) for exps in (good, high, low)}
        for k, exps in enumerate(runs):
            model = models[exps]
            sums, info = s.test_stan_sums(-1, beta, b, set_exp=exps)
            paths.append(check_exact(impl, True, sums, info, model, exps, f"hygiene evaluation {k}"))
            if exps == good:
                assert model["reject"] == 0
                if first is None:
                    first = (sums.copy(), info)
                same_bits(sums, first[0], f"hygiene evaluation {k}: the repeated evaluation")
                assert (info["mag"], info["exw"]) == (first[1]["mag"], first[1]["exw"])
            elif exps == high:
                assert model["reject"] & (REJECT_FLAG | REJECT_WORD) and not model["reject"] & REJECT_TINY
            else:
                assert model["reject"] == REJECT_TINY
        return paths, [("good" if e == good else "high" if e == high else "low") for e in runs]
    finally:
        s.free()


def run_plain_shape(lib, prefix, n, K, terms, L=None):
    """Case c, side by side: a shape without the fixed-point path through the same entry."""
    L = L or limits()
    args = shape_case(n=n, K=K, terms=terms, seed=43)
    br = expected_branch(None, args, L)
    assert not br["fused"]
    s, data, impl = open_case(lib, prefix, args)
    try:
        beta, b = small_coefficients(data.K, data.q, 43)
        for mode, bt, bb in ((0, None, None), (-1, beta, b)):
            model = exact_model(data, mode, bt, bb, (0, 0, 0), L)
            sums, info = s.test_stan_sums(mode, bt, bb, set_exp=(3, 4, 5))
            assert check_exact(impl, False, sums, info, model, (0, 0, 0), f"plain shape K = {K} mode {mode}") == "plain"
    finally:
        s.free()


def edge_cases():
    """Case d: name -> (plants per workgroup | "entry", [(group, exponent, verdict derived in the module docstring)])."""
    F, W, T = REJECT_FLAG, REJECT_WORD, REJECT_TINY
    return {
        "one-workgroup": ([PLANT_A], [(g, E, v) for g in range(3) for E, v in ((11, 0), (12, (F | W) if g < 2 else W), (-26, 0), (-27, T))]),
        "partial-at-2^42": ([PLANT_C], [(g, 11, (F | W) if g < 2 else W) for g in range(3)]),
        "two-workgroups-below": ([PLANT_A, PLANT_B], [(g, 10, 0) for g in range(3)]),
        "two-workgroups-at": ([PLANT_A, PLANT_A], [(g, 10, W) for g in range(3)]),
        "entry-at-2^42": ("entry", [(2, 21, 0), (2, 22, F)]),
    }


def run_edges(lib, prefix, name, L=None):
    L = L or limits()
    plants, points = edge_cases()[name]
    args = vector_case([1024.0, 1.0], z=[1024.0, 1.0]) if plants == "entry" else planted_case(plants)
    s, data, impl = open_case(lib, prefix, args)
    seen = []
    try:
        for g, E, verdict in points:
            exps = tuple(E if k == g else 0 for k in range(3))
            model = exact_model(data, 0, None, None, exps, L)
            assert model["reject"] == verdict, f"{name}: group {g} at exponent {E}: the model derives verdict {model['reject']}, the docstring {verdict}"
            sums, info = s.test_stan_sums(0, set_exp=exps)
            path = check_exact(impl, True, sums, info, model, exps, f"{name}: group {g} at exponent {E}")
            assert path == ("fused" if verdict == 0 and impl == "s4b" else "plain")
            if impl == "s4b" and verdict == REJECT_TINY:
                assert info["exp_after"][g] == E + (L["target"] - (L["ex_min"] - 1)), (name, g, E, info["exp_after"])
            seen.append((g, E, model["mag"], model["exw"]))
        return seen
    finally:
        s.free()


def scaled_args(s_exp, cancelling, n=600):
    """Case e: y = 2^s c with small integers c (mode 0: e = y); K = 1.  Not cancelling: x = 2 c, one grouping term of three levels with stored values
    sign(c): every product is positive, the totals are the sums of the magnitudes.  Cancelling: rows in pairs (c, x) = (k, 1), (k, -1): every
    workgroup partial of X'e is exactly 0 under a magnitude of 2^s sum |c|."""
    g = np.random.default_rng(9300000 + (s_exp % 1000))
    c = g.integers(1, 8, n).astype(np.float64) * g.choice([-1.0, 1.0], n)
    if cancelling:
        c[1::2] = c[0::2]
        x = np.ones(n)
        x[1::2] = -1.0
    else:
        x = 2.0 * c
    args = stan_shape_case(n, 1, [(3, 0)], 7990, 1, iters=(2, 4), trees=2, plain_init=True)
    y = np.ldexp(c, s_exp)
    args.y = y
    args.X = np.asfortranarray(x.reshape(n, 1))
    args.w = np.sign(c)
    # (the starting values belong to the response's scale: where the chain starts is not the subject, that create succeeds is)
    args.bart_offset_init = np.zeros(n)
    args.sigma_init = float(np.ldexp(4.0, s_exp))
    args.prior_scale_for_aux = float(np.ldexp(4.0, s_exp))
    return args


def run_adaptation(lib, prefix, s_exp, cancelling, L=None, beyond_clamp=False):
    """From reset scales, the same mode-0 evaluation again and again: every result exact on the path taken, the verdict of every evaluation the one the
    data and the exponents of its launch imply, acceptance within the derived budget, then stable.  Returns (evaluations until the first accepted one,
    budget)."""
    L = L or limits()
    args = scaled_args(s_exp, cancelling)
    s, data, impl = open_case(lib, prefix, args)
    try:
        at_reset = exact_model(data, 0, None, None, (0, 0, 0), L)
        out_of_range = bool(at_reset["reject"] & (REJECT_FLAG | REJECT_WORD))
        if at_reset["reject"] == 0:
            budget = 1
        else:
            budget = adaptation_budget(max(x for x in at_reset["top"] if x is not None), out_of_range, cancelling, L)
        if cancelling:
            assert exact_model(data, 0, None, None, (0, 0, 0), L)["total"][1] == 0.0
        first, exps, stable = None, (0, 0, 0), 0
        for k in range(1, (budget + 5) if not beyond_clamp else 8):
            sums, info = s.test_stan_sums(0, set_exp=(0, 0, 0) if k == 1 else None)
            if impl != "s4b":
                check_exact(impl, True, sums, info, at_reset, (0, 0, 0), f"scale 2^{s_exp} evaluation {k}")
                continue
            assert info["exp_used"] == tuple(exps), f"evaluation {k} was launched with {info['exp_used']}, the previous one left {exps}"
            model = exact_model(data, 0, None, None, exps, L)
            path = check_exact(impl, True, sums, info, model, exps, f"scale 2^{s_exp} evaluation {k}")
            assert all(abs(e) <= L["clamp"] for e in info["exp_after"])
            if beyond_clamp:
                assert path == "plain", f"evaluation {k} of an input beyond the clamp was accepted"
            elif path == "fused":
                if first is None:
                    first = k                                        # (this one centres the exponents on what it measured; the next ones find them centred)
                else:
                    assert info["exp_after"] == info["exp_used"], f"evaluation {k}: the exponents still move after acceptance: {info}"
                    stable += 1
            else:
                assert first is None, f"evaluation {k} was rejected after evaluation {first} had been accepted with the same input"
            exps = info["exp_after"]
        if impl == "s4b" and not beyond_clamp:
            assert first is not None and first <= budget, f"scale 2^{s_exp}: first accepted evaluation {first}, the documented rule allows {budget}"
            assert stable >= 2
        return first, budget
    finally:
        s.free()


def e_model_from_state(args, sv, mode):
    """(e in long double, its error bound per observation) of a mode-0 / mode-1 evaluation, formed from the state blob as handoff_cases.py forms its
    quantities.  Mode 0: e = y, exact.  Mode 1, continuous: the device forms yr - R (the blob's total fits F, the same expression in doubles; one
    rounding u |F| is allowed for the blob's own), fit = ((F + 1/2) range) + min (two roundings, or one when contracted) and e = y - fit (one).
    Binary: F = latent - R, response = latent + offset (one rounding), e = response - F (one)."""
    y = np.asarray(args.y, dtype=np.float64).astype(LD)
    if mode == 0:
        return y, np.zeros(len(y), LD)
    F = sv.get("total_fits").astype(LD)
    if sv.binary:
        resp = sv.get("latents").astype(LD) + sv.get("offset").astype(LD)
        e = resp - F
        return e, LD(U) * (np.abs(resp) + np.abs(F) + np.abs(e))
    mn, _, rng, _ = (LD(v) for v in sv.get("scale"))
    t = (F + LD(0.5)) * rng
    fit = t + mn
    e = y - fit
    return e, LD(U) * (np.abs(F) * rng + 2 * np.abs(t) + np.abs(fit) + np.abs(e))


def run_direct_against_indirect(lib, prefix, args, mode, report, L=None):
    """Case f: a !DIRECT evaluation (mode 0, or mode 1 after warm-up iterations and one hand-off with non-zero coefficients), then DIRECT with
    beta = b = 0 under the same exponents: bit-identical sums (the e0 the first one wrote is the e it summed); the sums within the bound of the
    long-double model of e."""
    from handoff_cases import state_view
    L = L or limits()
    s, data, impl = open_case(lib, prefix, args)
    try:
        if mode == 1:
            s.run(2, True)
            g = np.random.default_rng(77)
            s.test_hand_off(g.uniform(-1.0, 1.0, data.K), 0.7 * g.standard_normal(data.q), 0.9, False)
        sv = state_view(s)
        exps = None
        for _ in range(6):                                           # (find exponents this input is accepted with; the emulation has none)
            sums, info = s.test_stan_sums(mode)
            if info["accepted"] or impl != "s4b":
                exps = info["exp_used"]
                break
        assert exps is not None, "no accepted evaluation within 6"
        a, ia = s.test_stan_sums(mode, set_exp=exps)
        z, iz = s.test_stan_sums(-1, np.zeros(data.K), np.zeros(data.q), set_exp=exps)
        if impl == "s4b":
            assert ia["accepted"] and iz["accepted"], (ia, iz)
            assert (ia["mag"], ia["exw"]) == (iz["mag"], iz["exw"])
        same_bits(a, z, f"mode {mode} against DIRECT with zero coefficients")
        e, de = e_model_from_state(args, sv, mode)
        path = "fused" if impl == "s4b" else "serial"
        ref, bound = bounded_model(data, e, None, None, exps, path, de0=de, L=L)
        check_bounded(a, ref, bound, f"mode {mode}", report)
        if mode == 0 and impl == "s4b" and not args.is_binary:
            return exps
        return exps
    finally:
        s.free()


def run_bounded(lib, prefix, name, report, L=None):
    """Random data of a geometry case's shape: mode 0 (e = y) and DIRECT with random coefficients against the long-double model, on whichever path the
    evaluation took (asserted from info: the second evaluation of each kind must be on the fused path on the device)."""
    import zlib
    L = L or limits()
    spec = dict(geometry_cases(L)[name])
    seed = zlib.crc32(name.encode()) % 1000
    args = shape_case(seed=seed, exact=False, **{k: v for k, v in spec.items() if k != "empty_rows"})
    s, data, impl = open_case(lib, prefix, args)
    try:
        g = np.random.default_rng(seed)
        beta, b = g.uniform(-1.0, 1.0, data.K), 0.7 * g.standard_normal(data.q)
        paths = []
        for mode, bt, bb in ((0, None, None), (-1, beta, b)):
            for rep in range(3):
                sums, info = s.test_stan_sums(mode, bt, bb, set_exp=(0, 0, 0) if rep == 0 and mode == 0 else None)
                path = "fused" if info["accepted"] else ("plain" if impl == "s4b" else "serial")
                ref, bound = bounded_model(data, data.y, bt, bb, info["exp_used"], path, L=L)
                check_bounded(sums, ref, bound, f"{path}", report)
                paths.append(path)
            if impl == "s4b":
                assert paths[-1] == "fused", f"{name}: the third evaluation of mode {mode} was still rejected: {info}"
        if impl == "s4b":
            # the same evaluation with scales 70 bits too large: rejected for range, repeated in plain doubles, held to the plain pipeline's bound
            sums, info = s.test_stan_sums(-1, beta, b, set_exp=tuple(e + 70 for e in info["exp_used"]))
            assert not info["accepted"] and info["reject"] & (REJECT_FLAG | REJECT_WORD) and not info["reject"] & REJECT_TINY, info
            ref, bound = bounded_model(data, data.y, beta, b, info["exp_used"], "plain", L=L)
            check_bounded(sums, ref, bound, "plain", report)
            paths.append("plain")
        return paths
    finally:
        s.free()


def run_non_finite(lib, prefix, bad_value, L=None):
    """Case g: a finite accepted evaluation, one with a non-finite coefficient (rejected by the device's flag, ss not finite, the scales stay), a finite
    one again (accepted, exact)."""
    L = L or limits()
    args = shape_case(n=L["sblock"] + 44, K=2, terms=[(4, 0)], seed=47)
    s, data, impl = open_case(lib, prefix, args)
    try:
        beta, b = small_coefficients(data.K, data.q, 47)
        s.test_stan_sums(0, set_exp=(0, 0, 0))
        exps = centred_exps(data, -1, beta, b, L)
        model = exact_model(data, -1, beta, b, exps, L)
        sums, info = s.test_stan_sums(-1, beta, b, set_exp=exps)
        check_exact(impl, True, sums, info, model, exps, "before the non-finite evaluation")
        after = info["exp_after"]
        bad = beta.copy()
        bad[0] = bad_value
        sums, info = s.test_stan_sums(-1, bad, b)
        assert not np.isfinite(sums[0]), sums[0]
        assert not info["accepted"]
        if impl == "s4b":
            assert info["reject"] & REJECT_FLAG, info
            assert info["exp_used"] == after and info["exp_after"] == after, f"one evaluation out of range moved the scales: {info}"
        model = exact_model(data, -1, beta, b, after, L)
        sums, info = s.test_stan_sums(-1, beta, b)
        path = check_exact(impl, True, sums, info, model, after, "after the non-finite evaluation")
        assert path == ("fused" if impl == "s4b" else "plain")
    finally:
        s.free()


# Beyond the clamp: y = 2^470 c.  A workgroup's partial of ss is about 2^(940 + 12); the smallest exponent, -900, leaves 2^52 >= 2^42: out of range for ever.
# (The small side — ss below 2^-896 — is out of reach: Stan's initialisation fails on a response of 2^-456.)
BEYOND_CLAMP = 470
