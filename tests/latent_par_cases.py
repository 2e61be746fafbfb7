"""The parallel probit latents (latent mode 1: k_latents_par, stan4bart_amd/csrc/dev_hip.hip; the draw itself: philox_trunc_normal, csrc/philox.hpp;
DESIGN.md 5.4b) ALONE: an independent model of one draw, the key hash, the tools that edit a mode-1 state blob, the cases and the bounds shared by
tests/test_latents_par_alone.py (CPU: the model against the header compiled for the host, the cases' claims, the launch geometry) and
tests/test_gpu_latents_par_alone.py (the kernel against the model through s4b_test_draw_latents).

The model is written from Salmon et al. (2011) and DESIGN.md 5.4b, not from the header: Philox4x32-10 vectorised in numpy uint64 (every product of
two 32-bit words fits), counter = {draw index low, draw index high, observation, attempt}, key = {low half, high half} of the chain's 64-bit key; a
uniform is (m + 1/2) 2^-53 for the 53-bit m = (first word << 21) ^ (second word >> 11), formed in DOUBLE like the kernel's (m + 1/2 rounds to even
from 2^52 on: both sides see the same double); everything after the uniforms in np.longdouble (64-bit mantissa) from the double `lower` the
kernel sees:
    lower < 0:    rad = sqrt(-2 log u1), th = 2 pi u2 (2 pi the double 6.283185307179586); z0 = rad cos th is accepted if z0 >= lower, else
                  z1 = rad sin th if z1 >= lower, else the next attempt;
    lower >= 0:   lam = (lower + sqrt(lower^2 + 4)) / 2, z = lower - log(u1) / lam, accepted if u2 <= exp(-(z - lam)^2 / 2)   (Robert 1995).
lower = -(fits + offset) for y = 1 and fits + offset for y = 0 (-0.0 is not below 0: it takes the second branch); the stored latent is
(mean + x) - offset for y = 1 and (mean - x) - offset for y = 0.  Per observation the model returns the deviate, the number of attempts, the
accepted deviate (0: z0, 1: z1, 2: exponential proposal), the smallest MARGIN of any comparison it made (|z - lower|, |u2 - exp(.)|), and the
bounds below.  Domain: lower^2 finite in double (|mean| below sqrt(DBL_MAX), about 1.3e154; the model's long double would not overflow there, the
kernel's lam does: `failure_lower`, never part of cases()).

BOUNDS, u = 2^-53, derived and not fitted; k_f is the error of the library function f in ulps (an error of k ulps is at most 2 k u relative).
  DEVICE  log 1, exp 1, sin / cos 2, sqrt 1: ASSUMED — the figures the HIP programming guide's table of double-precision math functions gives;
          no copy of that table is installed with the toolchain the suite builds with, so nothing here reads it.
  GLIBC   1 ulp each (the host comparison of the CPU file).
  normal branch      log(u1) is off by 2 k_log u relative; the factor -2 is exact; the square root halves that and adds its own 2 k_sqrt u:
                     rad is off by (k_log + 2 k_sqrt) u relative.  th = fl(2 pi u2) is off by 0.5 ulp, at most u th <= 2 pi u absolute, which moves
                     cos / sin by at most as much: 2 pi u rad in the product.  cos / sin add 2 k_trig u relative to their result, the product
                     rounds once (u |x|):
                         |x error| <= u (C1 rad + C2 |x|),   C1 = 2 pi,   C2 = k_log + 2 k_sqrt + 2 k_trig + 1        (device 8, glibc 6).
  exponential branch s = lower^2 + 4 in two roundings or one (the device contracts lower * lower + 4 to an FMA; both stay within 2 u relative, all
                     terms being positive); sqrt: u + 2 k_sqrt u; lower + sqrt(s) adds one rounding of a sum of non-negative terms, the half is
                     exact: lam is off by C_LAM u relative, C_LAM = 2 + 2 k_sqrt = 4.  E = -log(u1): 2 k_log u; the (correctly rounded)
                     quotient E / lam: (2 k_log + C_LAM + 1) u relative; the sum lower + E / lam rounds once:
                         |x error| <= u (|x| + C3 E / lam) + p <= (C3 + 1) u (|lower| + E / lam) + p,   C3 = 2 k_log + C_LAM + 1 = 7,
                     p the perturbation of lower (below; dx / dlower is 1 - (E / lam^2) dlam / dlower, between 0 and 1).
                     The acceptance compares u2 (exact) with exp(e), e = -d^2 / 2, d = z - lam:  |d error| <= |x error| + C_LAM u lam + p + u |d|,
                     e is off by |d| |d error| + u |e| (two products), exp(e) by exp(e) (|e error| + 2 k_exp u).
  lower              mean = fl(fOld + offset), fOld = fl(latent - R): the model forms both in double from the blob's doubles exactly as the kernel does
                     (first draw: inputs on the 2^-20 grid, R = latent - fits and fOld = latent - R are exact; second draw: the blob's total_fits IS
                     fl(latent - R), the kernel's fOld), so p would be 0.  One rounding of each is allowed all the same:
                         p = u (|fits| + |mean|).
  stored latent      z = fl(mean +- x) and nl = fl(z - offset) round once each:  |latent error| <= |x error| + p + u (|z| + |nl|), |nl| <= |z| + |offset|.
  total_fits         the blob's fl(nl - R') with R' = fl(nl - fOld) against fOld: 2 u max(|latent|, |fits|) of the state after the draw.
Every comparison with the model allows BOUND_FACTOR = 4 times its bound (readout_cases / handoff_cases: the reference's own roundings and its
conversion to double).  A decision is UNDECIDED when its margin is below 4 times the bound of the compared quantity (plus p for z >= lower; p is
inside the acceptance bound).  Condition on the inputs, asserted by the builder: NO undecided observation in either of the two consecutive draws of
any case, under the device's figures (the wider ones).  Random cases are re-seeded until it holds (`_retry`); nothing is left out at run time.

GEOMETRY (dev_hip.hip, read by `kernel_geometry`): workgroups = min(1024, ceil(ceil(n / 4) / BLOCK)), BLOCK = 256 threads; observation i belongs
to trip i // (workgroups * BLOCK) of thread i % (workgroups * BLOCK).  A latent depends on (key, draw index, i, mean) only."""
import os
import re

import numpy as np

from latent_cases import _quant
from readout_cases import BOUND_FACTOR, U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stan4bart_amd", "csrc")
LD = np.longdouble
TWO_PI = 6.283185307179586
MAX_ATTEMPTS = 4096
DEVICE = dict(log=1.0, exp=1.0, trig=2.0, sqrt=1.0)         # ASSUMED (module docstring)
GLIBC = dict(log=1.0, exp=1.0, trig=1.0, sqrt=1.0)
C_FITS = 2.0
_M32 = np.uint64(0xFFFFFFFF)


# ---- the generator ---------------------------------------------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32 with ten rounds (Salmon et al. 2011, section 3.3 / Random123): per round (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2),
    hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key bumped by the two Weyl constants between rounds.  Counter words: arrays or scalars; four uint64 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _M32
    return c0, c1, c2, c3


def u53(hi, lo):
    """The midpoint of the 53-bit cell, formed in double."""
    m = (hi << np.uint64(21)) ^ (lo >> np.uint64(11))
    return (m.astype(np.float64) + 0.5) * 2.0 ** -53


def latent_key(rstate, seed):
    """The chain's 64-bit Philox key (SamplerCore::latent_key restated): a splitmix64-style finaliser folded over the Stan seed and the 625 words of
    R's generator state the chain was created with."""
    m64 = (1 << 64) - 1

    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & m64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m64
        return z ^ (z >> 31)
    h = mix(int(seed) & 0xFFFFFFFF)
    for w in np.asarray(rstate, dtype=np.uint32)[:625].tolist():
        h = mix(h ^ w)
    return h


def sampler_key(seed=12345):
    """The key of conftest.make_sampler(lib, prefix, args, seed): its Stan seed is the first sample.int of RRng(seed), the state the one after it."""
    from stan4bart_amd import RRng
    rng = RRng(seed)
    stan_seed = int(rng.sample_int(2147483647, 1)[0])
    return latent_key(rng.state, stan_seed)


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------------
def lower_of(y, offset, fold):
    """(mean, lower, perturbation bound of lower) in double, as the kernel forms them from fOld = latent - R."""
    mean = np.asarray(fold, dtype=np.float64) + np.asarray(offset, dtype=np.float64)
    lower = np.where(np.asarray(y) > 0.0, 0.0 - mean, mean - 0.0)
    return mean, lower, U * (np.abs(fold) + np.abs(mean))


def draw(key, index, lower, pert=None, obs=None):
    """One draw for the observations `obs` (default 0..n-1) with the bounds `lower` (double) under (key, draw index).  Returns a dict of arrays:
    x (long double), attempts, branch (0 z0, 1 z1, 2 exponential), margin, undecided (under the DEVICE figures), bound['device' | 'glibc'] of x."""
    lower = np.asarray(lower, dtype=np.float64)
    n = lower.size
    assert np.all(np.abs(lower) < 1e150), "outside the model's domain: lower^2 must be finite in double"
    pert = np.zeros(n) if pert is None else np.asarray(pert, dtype=np.float64)
    obs = np.arange(n, dtype=np.uint64) if obs is None else np.asarray(obs, dtype=np.uint64)
    k0, k1 = int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF
    d0, d1 = int(index) & 0xFFFFFFFF, (int(index) >> 32) & 0xFFFFFFFF
    x = np.zeros(n, dtype=LD); attempts = np.zeros(n, dtype=np.int64); branch = np.full(n, -1, dtype=np.int64)
    margin = np.full(n, np.inf); undecided = np.zeros(n, dtype=bool)
    bound = {"device": np.zeros(n), "glibc": np.zeros(n)}
    tabs = (("device", DEVICE), ("glibc", GLIBC))
    neg = lower < 0.0
    act_n, act_e = np.nonzero(neg)[0], np.nonzero(~neg)[0]
    for t in range(MAX_ATTEMPTS):
        if act_n.size == 0 and act_e.size == 0:
            break
        if act_n.size:
            I = act_n
            r = philox4x32_10(d0, d1, obs[I], t, k0, k1)
            u1, u2 = u53(r[0], r[1]), u53(r[2], r[3])
            lo, p = lower[I].astype(LD), pert[I]
            rad = np.sqrt(LD(-2.0) * np.log(u1.astype(LD)))
            th = LD(TWO_PI) * u2.astype(LD)
            z = (rad * np.cos(th), rad * np.sin(th))
            b = {name: [U * (TWO_PI * rad.astype(np.float64) + (k["log"] + 2 * k["sqrt"] + 2 * k["trig"] + 1) * np.abs(zz).astype(np.float64)) for zz in z]
                 for name, k in tabs}
            m0 = np.abs(z[0] - lo).astype(np.float64)
            m1 = np.abs(z[1] - lo).astype(np.float64)
            a0 = z[0] >= lo
            a1 = ~a0 & (z[1] >= lo)
            margin[I] = np.minimum(margin[I], np.where(a0, m0, np.minimum(m0, m1)))
            undecided[I] |= (m0 < BOUND_FACTOR * b["device"][0] + p) | (~a0 & (m1 < BOUND_FACTOR * b["device"][1] + p))
            for which, acc in ((0, a0), (1, a1)):
                J = I[acc]
                x[J] = z[which][acc]; attempts[J] = t + 1; branch[J] = which
                for name, _ in tabs:
                    bound[name][J] = b[name][which][acc]
            act_n = I[~(a0 | a1)]
        if act_e.size:
            I = act_e
            r = philox4x32_10(d0, d1, obs[I], t, k0, k1)
            u1, u2 = u53(r[0], r[1]), u53(r[2], r[3])
            lo, p = lower[I].astype(LD), pert[I]
            lam = LD(0.5) * (lo + np.sqrt(lo * lo + LD(4.0)))
            tt = -np.log(u1.astype(LD)) / lam
            z = lo + tt
            d = z - lam
            e = LD(-0.5) * d * d
            pr = np.exp(e)
            f = [np.asarray(v, dtype=np.float64) for v in (np.abs(z), tt, lam, np.abs(d), np.abs(e), pr)]
            b, bp = {}, {}
            for name, k in tabs:
                clam = 2.0 + 2.0 * k["sqrt"]
                b[name] = U * (f[0] + (2.0 * k["log"] + clam + 1.0) * f[1]) + p
                derr = b[name] + clam * U * f[2] + p + U * f[3]
                bp[name] = f[5] * (f[3] * derr + U * f[4] + 2.0 * k["exp"] * U)
            m = np.abs(u2.astype(LD) - pr).astype(np.float64)
            acc = u2.astype(LD) <= pr
            margin[I] = np.minimum(margin[I], m)
            undecided[I] |= m < BOUND_FACTOR * bp["device"]
            J = I[acc]
            x[J] = z[acc]; attempts[J] = t + 1; branch[J] = 2
            for name, _ in tabs:
                bound[name][J] = b[name][acc]
            act_e = I[~acc]
    assert act_n.size == 0 and act_e.size == 0, "an observation found no proposal in 4 096 attempts"
    return dict(x=x, attempts=attempts, branch=branch, margin=margin, undecided=undecided, bound=bound)


def store(y, offset, fold, x):
    """What the kernel stores for the deviates x (double), restated in double: (new latents, new R, the total_fits a blob then reports)."""
    mean = np.asarray(fold, dtype=np.float64) + offset
    z = np.where(y > 0.0, mean + x, mean - x)
    nl = z - offset
    R = nl - fold
    return nl, R, nl - R


def latent_of(y, offset, fold, m, pert):
    """(stored latent of the model, long double; its bound under the device's figures) for a draw m of the model."""
    mean = (np.asarray(fold, dtype=np.float64) + offset).astype(LD)
    z = np.where(y > 0.0, mean + m["x"], mean - m["x"])
    nl = z - np.asarray(offset, dtype=LD)
    return nl, m["bound"]["device"] + pert + U * (np.abs(z) + np.abs(nl)).astype(np.float64)


def mp_draw(key, index, obs, lower, digits=40):
    """The same draw for ONE observation in mpmath at `digits` digits: (x, attempts, branch)."""
    import mpmath as mp
    k0, k1 = int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF
    with mp.workdps(digits):
        lo = mp.mpf(float(lower))
        for t in range(MAX_ATTEMPTS):
            r = philox4x32_10(int(index) & 0xFFFFFFFF, (int(index) >> 32) & 0xFFFFFFFF, int(obs), t, k0, k1)
            u1, u2 = (mp.mpf(float(u53(r[0], r[1]))), mp.mpf(float(u53(r[2], r[3]))))
            if float(lower) < 0.0:
                rad, th = mp.sqrt(-2 * mp.log(u1)), mp.mpf(TWO_PI) * u2
                for which, zz in ((0, rad * mp.cos(th)), (1, rad * mp.sin(th))):
                    if zz >= lo:
                        return zz, t + 1, which
            else:
                lam = (lo + mp.sqrt(lo * lo + 4)) / 2
                zz = lo - mp.log(u1) / lam
                if u2 <= mp.exp(-(zz - lam) ** 2 / 2):
                    return zz, t + 1, 2
    raise AssertionError("no proposal accepted")


# ---- geometry --------------------------------------------------------------------------------------------------------------------------------------------
def kernel_geometry(src_path=None, philox_path=None):
    """BLOCK and the workgroup cap READ from dev_hip.hip, with the statements the cases rest on asserted to still be there: the grid line, the launch
    line that passes the key halves and the draw index, the advance of the draw index beside it, the kernel's observation word and grid-stride loop,
    and the counter initialiser of philox.hpp."""
    src = open(src_path or os.path.join(CSRC, "dev_hip.hip")).read()
    phx = open(philox_path or os.path.join(CSRC, "philox.hpp")).read()
    block = int(re.search(r"constexpr int BLOCK = (\d+);", src).group(1))
    m = re.search(r"a\.grid = \(int\)std::min<int64_t>\((\d+), std::max<int64_t>\(1, \(nQuads \+ BLOCK - 1\) / BLOCK\)\);", src)
    assert m, "the grid line of the O(N) kernels changed"
    assert "const int64_t nQuads = (n_ + 3) / 4;" in src and "gridN_ = a.grid;" in src
    assert "hipLaunchKernelGGL(k_latents_par, dim3(gridN_), dim3(BLOCK), 0, stream_, a_, (uint32_t)latKey_, (uint32_t)(latKey_ >> 32), latDraw_);\n      ++latDraw_; ++launches_;" in src, \
        "the launch line of k_latents_par changed"
    assert "for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * BLOCK) {\n    const double fOld = a.lat[i] - a.R[i], offv = a.off[i], mean = fOld + offv;\n    const bool one = a.y[i] > 0.0;" in src
    assert "philox_trunc_normal(k0, k1, draw, (uint32_t)i, one ? 0.0 - mean : mean - 0.0, x);" in src, "the observation word of k_latents_par changed"
    assert "Philox4 c = {{(uint32_t)draw, (uint32_t)(draw >> 32), obs, 0u}};" in phx, "the counter layout of philox.hpp changed"
    assert phx.count("c.v[3] = (uint32_t)t;") == 2 and "constexpr int TN_MAX_ATTEMPTS = 1 << 12;" in phx
    return dict(block=block, cap=int(m.group(1)))


def geometry(n, lim):
    """(workgroups, trips of the grid-stride loop, observations in the last trip) of k_latents_par at n."""
    quads = (n + 3) // 4
    grid = min(lim["cap"], max(1, (quads + lim["block"] - 1) // lim["block"]))
    threads = grid * lim["block"]
    trips = (n + threads - 1) // threads
    return grid, trips, n - (trips - 1) * threads


# hand-written: n -> (workgroups, trips, observations in the last trip), for BLOCK = 256 and a cap of 1 024 workgroups
GEOMETRY = {1: (1, 1, 1), 24: (1, 1, 24), 100: (1, 1, 100), 255: (1, 1, 255), 256: (1, 1, 256), 257: (1, 2, 1), 1000: (1, 4, 232), 1024: (1, 4, 256),
            1025: (2, 3, 1), 65537: (65, 4, 15617), 262147: (257, 4, 64771), 1048577: (1024, 5, 1)}


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------------
OWN_KEY = "own"          # the key the sampler reports itself (conftest.make_sampler's default seed): the tail's key is left untouched
SHARED_KEY = 0x6A09E667F3BCC908
SHARED_DRAW = (1 << 63) + 5


class Case:
    """name, n; y; offset, fits, lat (the state to inject); key (an integer or OWN_KEY), index (the draw index injected); claim (what the case says it
    hits: checked against the model's counts); m1, m2 (the model's two consecutive draws, the second from the state `store` leaves with the model's
    rounded deviates) with their means and perturbations (f1 / f2: the fOld each draw sees)."""

    def __init__(self, name, y, offset, fits, lat, key, index, claim=None, raw=None):
        self.name, self.n = name, len(y)
        self.y = np.asarray(y, dtype=np.float64)
        self.offset, self.fits, self.lat = _quant(offset), _quant(fits), _quant(lat)
        for k, (f, o, l) in (raw or {}).items():          # rows that are NOT on the 2^-20 grid: exact all the same (latent = offset = 0 or the like)
            self.fits[k], self.offset[k], self.lat[k] = f, o, l
        self.key, self.index = key, int(index)
        self.claim = dict(claim or {})
        key = self.key_value()
        self.f1 = self.lat - (self.lat - self.fits)
        assert np.array_equal(self.f1, self.fits), "latent - (latent - fits) is not fits"          # (the model goes on from f1: a fit of -0.0 arrives as +0.0)
        self.m1 = self.model(key, self.index, self.f1)
        nl, _, self.f2 = store(self.y, self.offset, self.f1, self.m1["x"].astype(np.float64))
        self.lat2 = nl
        self.m2 = self.model(key, (self.index + 1) & ((1 << 64) - 1), self.f2)

    def key_value(self):
        return sampler_key() if self.key == OWN_KEY else int(self.key)

    def model(self, key, index, fold):
        mean, lower, pert = lower_of(self.y, self.offset, fold)
        m = draw(key, index, lower, pert)
        m["mean"], m["lower"], m["pert"] = mean, lower, pert
        return m

    def counts(self, m):
        """(normal branch: >= 2 attempts, >= 3 attempts; exponential branch: >= 2, >= 3; accepted on the second deviate)"""
        nb, eb, a = m["branch"] < 2, m["branch"] == 2, m["attempts"]
        return (int((nb & (a >= 2)).sum()), int((nb & (a >= 3)).sum()), int((eb & (a >= 2)).sum()), int((eb & (a >= 3)).sum()), int((m["branch"] == 1).sum()))

    def undecided(self):
        return int(self.m1["undecided"].sum() + self.m2["undecided"].sum())

    def __repr__(self):
        return self.name


def _retry(make, what, need_counts):
    for attempt in range(64):
        c = make(attempt)
        if c.undecided() == 0 and (not need_counts or (min(c.counts(c.m1)) >= 1 and min(c.counts(c.m2)) >= 1)):
            return c
    raise AssertionError(f"no draw of case {what} keeps every decision away from a tie and reaches every branch")


def _mixed_means(g, n, ys):
    """(y, offset, fits): half of the observations with means uniform on [-8, 8] (a user offset), the other half with means 0.4 N(0, 1) (bounds near 0:
    where both branches reject most), small fits under both; y independent of the means: 'mixed' Bernoulli(1/2), 'ones', 'zeros'."""
    near = g.random(n) < 0.5
    off = np.where(near, 0.4 * g.standard_normal(n), g.uniform(-8.0, 8.0, n))
    fits = 0.25 * g.standard_normal(n)
    y = {"mixed": (g.random(n) < 0.5).astype(np.float64), "ones": np.ones(n), "zeros": np.zeros(n)}[ys]
    return y, off, fits


def random_case(name, n, key, index, ys="mixed", seed=0, prefix=None):
    """A random case; `prefix` = (y, offset, fits, lat) of the shared first observations (geometry independence)."""
    def make(attempt):
        g = np.random.default_rng([seed, attempt, n])
        y, off, fits = _mixed_means(g, n, ys)
        lat = g.standard_normal(n)
        if prefix is not None:
            k = len(prefix[0])
            y[:k], off[:k], fits[:k], lat[:k] = prefix
        return Case(name, y, off, fits, lat, key, index, dict(n=n, index=index, key=key if key == OWN_KEY else hex(key), y=ys))
    return _retry(make, name, n >= 256)


def bounds_case():
    """The named bounds, three observations each (other observation words, other random numbers): lower = +0.0 (y = 1, mean 0), -0.0 (y = 0, mean
    -0.0: latent = fits = offset = -0.0, and -0.0 is not below 0), -1e-300, -8, 8, -40, 40, 1e8."""
    rows = [(1.0, 0.0, False), (0.0, -0.0, False), (1.0, 1e-300, True), (1.0, 8.0, False), (0.0, 8.0, False), (1.0, 40.0, False), (0.0, 40.0, False),
            (0.0, 1e8, True)]
    lowers = [0.0, -0.0, -1e-300, -8.0, 8.0, -40.0, 40.0, 1e8]

    def make(attempt):
        n = 3 * len(rows)
        y, fits, off, lat, raw = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), {}
        for j in range(n):
            yy, mean, is_raw = rows[j % len(rows)]
            y[j] = yy
            if is_raw:
                raw[j] = (mean, 0.0, 0.0)
            elif mean == 0.0:
                raw[j] = (mean, mean, mean)
            else:
                fits[j] = mean
        c = Case("bounds-n24", y, off, fits, lat, 0x0123456789ABCDEF + attempt, SHARED_DRAW, dict(lowers=lowers), raw=raw)
        assert np.array_equal(c.m1["lower"][:8], lowers) and np.array_equal(np.signbit(c.m1["lower"][:8]), np.signbit(lowers))
        assert np.array_equal(c.m1["branch"][:8] == 2, [True, True, False, False, True, False, True, True])
        return c
    return _retry(make, "bounds-n24", False)


def convention_case():
    """Offsets of order 1e3 under means of order 1, previous latents unrelated to either: latent - R, + offset, - offset do not cancel."""
    def make(attempt):
        g = np.random.default_rng([13, attempt])
        n = 100
        off = np.clip(1e3 * g.standard_normal(n), -4000.0, 4000.0)
        mean = 1.5 * g.standard_normal(n)
        y = (mean + g.standard_normal(n) > 0.0).astype(np.float64)
        return Case("conventions-offset-1e3", y, off, _quant(mean) - _quant(off), 30.0 * g.standard_normal(n), 0xFFFFFFFF00000001, 2, dict(offset_scale=1e3))
    return _retry(make, "conventions-offset-1e3", False)


# what every case with n >= 256 reaches, stated and asserted (tests/test_latents_par_alone.py): observations of the first and of the second draw with
# (>= 2, >= 3 attempts on the normal branch; >= 2, >= 3 attempts on the exponential branch; the second Box-Muller deviate accepted)
CLAIMS = {
    "n1-own-key-draw0": ((0, 0, 0, 0, 0), (0, 0, 0, 0, 0)),
    "n255-key-low0-draw1-ones": ((16, 3, 10, 0, 20), (9, 0, 14, 2, 24)),
    "n256-key-high0-draw-2p32m1-zeros": ((5, 2, 13, 2, 19), (5, 1, 13, 3, 27)),
    "n257-key-ones-draw-2p32": ((14, 2, 13, 3, 11), (5, 2, 10, 1, 23)),
    "n1000-shared": ((44, 11, 63, 6, 51), (41, 5, 53, 11, 84)),
    "n1024-draw0": ((35, 5, 63, 6, 79), (24, 5, 53, 11, 58)),
    "n1025-shared": ((45, 11, 64, 6, 52), (42, 5, 55, 12, 88)),
    "n65537-shared": ((2449, 442, 3903, 674, 4674), (2540, 436, 4040, 764, 4933)),
    "n262147-draw-2p32m1": ((10187, 1688, 15720, 2820, 19598), (9967, 1675, 15773, 2852, 19871)),
    "bounds-n24": ((1, 1, 1, 0, 0), (0, 0, 3, 2, 0)),
    "conventions-offset-1e3": ((3, 0, 2, 0, 10), (5, 2, 1, 0, 10)),
    "n1048577-own-key-draw1": ((40033, 6572, 62894, 11334, 78142), (40152, 6606, 63197, 11083, 78093)),
}

_TRI = "n1000-shared"


def _shared(name, n, seed):
    def build():
        tri = case(_TRI)
        return random_case(name, n, SHARED_KEY, SHARED_DRAW, seed=seed, prefix=(tri.y, tri.offset, tri.fits, tri.lat))
    return build


# name -> builder; a case is built when a test first asks for it (`case`), so that collecting the tests builds none
_BUILDERS = {
    "n1-own-key-draw0": lambda: random_case("n1-own-key-draw0", 1, OWN_KEY, 0, seed=1),
    "n255-key-low0-draw1-ones": lambda: random_case("n255-key-low0-draw1-ones", 255, 0xC2B2AE3D00000000, 1, ys="ones", seed=2),
    "n256-key-high0-draw-2p32m1-zeros": lambda: random_case("n256-key-high0-draw-2p32m1-zeros", 256, 0x0000000085EBCA6B, (1 << 32) - 1, ys="zeros", seed=3),
    "n257-key-ones-draw-2p32": lambda: random_case("n257-key-ones-draw-2p32", 257, (1 << 64) - 1, 1 << 32, seed=4),
    _TRI: lambda: random_case(_TRI, 1000, SHARED_KEY, SHARED_DRAW, seed=5),
    "n1024-draw0": lambda: random_case("n1024-draw0", 1024, 0x9E3779B97F4A7C15, 0, seed=6),
    "n1025-shared": _shared("n1025-shared", 1025, 7),
    "n65537-shared": _shared("n65537-shared", 65537, 8),
    "n262147-draw-2p32m1": lambda: random_case("n262147-draw-2p32m1", 262147, 0x243F6A8885A308D3, (1 << 32) - 1, seed=9),
    "bounds-n24": bounds_case,
    "conventions-offset-1e3": convention_case,
    "n1048577-own-key-draw1": lambda: random_case("n1048577-own-key-draw1", 1048577, OWN_KEY, 1, seed=10),      # (the one case that takes seconds to build)
}
CASE_NAMES = tuple(_BUILDERS)
CASE_N = {"bounds-n24": 24, "conventions-offset-1e3": 100, **{k: int(k.split("-")[0][1:]) for k in _BUILDERS if k[0] == "n"}}
assert set(CLAIMS) == set(CASE_NAMES)
_CASES = {}


def case(name):
    """The case of that name, built once per process."""
    if name not in _CASES:
        c = _BUILDERS[name]()
        assert c.name == name and c.n == CASE_N[name]
        _CASES[name] = c
    return _CASES[name]


def cases():
    """All cases."""
    return [case(name) for name in CASE_NAMES]


TRIPLE = ("n1000-shared", "n1025-shared", "n65537-shared")


def failure_lower():
    """OUTSIDE the domain, never part of cases(): y = 0 and mean 1e200, finite (set_state accepts it), lower^2 = inf, lam = inf, every proposal equals
    lower - log(u1) / inf = lower, z - lam = -inf and the acceptance probability is exp(-inf) = 0 for all 4 096 attempts."""
    return 1e200


# ---- a mode-1 state blob ---------------------------------------------------------------------------------------------------------------------------------
class ParState:
    """A state blob written in latent mode 1: what conftest.StateView parses, then 16 bytes {key, draw index}."""

    def __init__(self, blob, StateView):
        assert int(np.frombuffer(blob, dtype=np.int64, count=1, offset=40)[0]) == 1, "not a latent mode 1 state"
        self.sv = StateView(blob[:-16])
        self.key, self.index = (int(v) for v in np.frombuffer(blob[-16:], dtype=np.uint64))

    def bytes(self):
        return self.sv.bytes() + np.array([self.key, self.index], dtype=np.uint64).tobytes()

    def rest(self):
        """The blob with latents, total_fits and the draw index blanked: what a latent draw must leave bit-identical (the key included)."""
        b = bytearray(self.sv.bytes())
        for name in ("latents", "total_fits"):
            o, cnt, _ = self.sv.off[name]
            b[o:o + 8 * cnt] = bytes(8 * cnt)
        return bytes(b) + np.array([self.key], dtype=np.uint64).tobytes()


def sampler_args(case, thin=1):
    """A small probit sampler in latent mode 1 with the case's response (fixed at creation; the rest goes in through set_state)."""
    from stan4bart_amd import make_sampler_args
    g = np.random.default_rng(5)
    xb = np.asfortranarray(g.random((case.n, 2)))
    X = g.random((case.n, 1))
    return make_sampler_args(case.y, xb, X=X, family="binomial", iter=4, warmup=2, skip=(thin, 1), bart_args={"n.trees": 2, "latents": "parallel"})


def inject(sampler, case, StateView):
    """The case's state into a mode-1 sampler; returns the ParState injected."""
    ps = ParState(sampler.get_state(), StateView)
    assert ps.sv.binary and ps.sv.n == case.n
    ps.sv.set("offset", case.offset); ps.sv.set("total_fits", case.fits); ps.sv.set("latents", case.lat)
    if case.key != OWN_KEY:
        ps.key = int(case.key)
    ps.index = case.index
    sampler.set_state(ps.bytes())
    return ps
