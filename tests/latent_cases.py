"""The exact probit latents (latent mode 0: k_latents2 + k_latents_finish, stan4bart_amd/csrc/dev_hip.hip) ALONE, on streams the test
chooses: a plain serial model of the draw, the tools that craft a generator state, and the cases shared by tests/test_latents_exact.py (CPU: model,
oracle, emulated device layer) and tests/test_gpu_latents_exact.py (the kernel against the oracle through s4b_test_draw_latents).

The model (`draw`) is dbarts' sequential truncated-normal draw in Python doubles over the position-indexed stream of R's Mersenne-Twister: unif_rand's
mapping, norm_rand by inversion (rcompat.qnorm), exp_rand (Ahrens & Dieter), the two rejection loops.  It returns per observation the deviate, the
stream positions consumed and the smallest DECISION MARGIN — |x - lower| of every normal examined, |u - exp(-d^2 / 2)| of every exponential proposal,
|u - q_i| inside exp_rand.  The CPU test pins the model to the oracle on every case.

Condition on the inputs: every case has a smallest margin of at least MIN_MARGIN = 1e-9 (the project's absolute tolerance for floats) over BOTH
consecutive draws the tests make.  The device's exp / log / sqrt differ from libm by ulps; a case closer than that to a tie would test the maths
library, not the kernel.  The comparisons with q_i inside exp_rand() are kept apart (`qmargin`): their left side is the 32-bit output scaled by 2^-32,
doubled and reduced by one — exact in any IEEE arithmetic, no library call — so no distance from q_i can make two implementations disagree.  They are
held to MIN_MARGIN all the same, except in the cases that choose the outputs 0x80000000 and 0xFFFFFFFF (`exact_q` in their claims): the first gives
v = 1.0, one ulp above q[14] = 0.9999999999999999 — that closeness IS the 17-position exp_rand() the case is there for —, the second v = 1 - 2^-31,
6e-12 above q[9].
Random cases are re-seeded until they meet it, crafted ones re-draw their filler words; nothing is skipped at run time.

Domain: the kernel's table of next-slacks is 8 bit wide, so one observation may consume at most 256 stream positions (127 rejected normals);
exactly 128 rejections is the edge of the domain and stays OUT of every case (`MAX_POSITIONS`, asserted by the builder for every observation).

Inputs are multiples of 2^-20 below 2^12 in magnitude, so that latent - (latent - fits) == fits holds exactly: the emulated device layer and the
kernel keep the residual latent - fits where the oracle keeps the fits, and with such inputs all three see the same mean bit for bit in the first draw."""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_MARGIN = 1e-9
MAX_POSITIONS = 256
BIG = 134217728.0
SIZES = (4, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4096, 4097)
START_MTI = (1, 2, 623, 624)
Q = (0.6931471805599453, 0.9333736875190459, 0.9888777961838675, 0.9984589039328340, 0.9998292811061389, 0.9999833164100727, 0.9999985691438767,
     0.9999998906925558, 0.9999999924734159, 0.9999999995283275, 0.9999999999728814, 0.9999999999985598, 0.9999999999999289, 0.9999999999999968,
     0.9999999999999999, 1.0000000000000000)


def kernel_limits():
    """L_NB (observations per batch), L_CH (per chunk), L_RING, L_BLK, L_EMAX READ from dev_hip.hip, with the statements the claims below rest on."""
    src = open(os.path.join(ROOT, "stan4bart_amd", "csrc", "dev_hip.hip")).read()
    m = re.search(r"constexpr int L_RING = (\d+), L_CH = (\d+), L_NB = S4B_L_NB, L_BLK = (\d+), L_EMAX = (\d+);", src)
    nb = int(re.search(r"#define S4B_L_NB (\d+)", src).group(1))
    assert "S.T[i][lane] = (bad || sl > 254) ? (uint8_t)255 : (uint8_t)sl;" in src and "alive = take & (nx < 64 ? 1 : 0);" in src
    return dict(ring=int(m.group(1)), ch=int(m.group(2)), nb=nb, blk=int(m.group(3)), emax=int(m.group(4)))


# ---- Mersenne-Twister: tempering and its inverse, one block forwards and backwards ---------------------------------------------------------------------
def temper(y):
    y = np.asarray(y, dtype=np.uint32).copy()
    y ^= y >> np.uint32(11)
    y ^= (y << np.uint32(7)) & np.uint32(0x9D2C5680)
    y ^= (y << np.uint32(15)) & np.uint32(0xEFC60000)
    y ^= y >> np.uint32(18)
    return y


def untemper(z):
    """The state word whose tempered output is z (every step of the tempering is a bijection of the 32-bit words)."""
    out = np.empty(np.shape(z), dtype=np.uint32)
    flat = np.asarray(z, dtype=np.uint32).reshape(-1)
    res = out.reshape(-1)
    for k, v in enumerate(flat.tolist()):
        y = v ^ (v >> 18)
        y ^= (y << 15) & 0xEFC60000
        t = y
        for _ in range(5):                       # y = t ^ ((y << 7) & mask): seven more bits are right after every pass
            y = t ^ ((y << 7) & 0x9D2C5680)
        y &= 0xFFFFFFFF
        t = y
        for _ in range(3):
            y = t ^ (y >> 11)
        res[k] = y & 0xFFFFFFFF
    return out


_UP, _LO, _A = 0x80000000, 0x7FFFFFFF, 0x9908B0DF


def _twist(y):
    return (y >> 1) ^ (_A if (y & 1) else 0)


def _untwist(t):
    """y of _twist(y) = t: the matrix constant has its top bit set and y >> 1 has not, so the top bit of t is y's lowest bit."""
    return (((t ^ _A) << 1) | 1) & 0xFFFFFFFF if (t & _UP) else (t << 1) & 0xFFFFFFFF


def mt_forward(mt):
    """The next block of 624 state words (R's MT_genrand regeneration, plain integers)."""
    m = [int(v) for v in mt]
    for k in range(624):
        y = (m[k] & _UP) | (m[(k + 1) % 624] & _LO)
        m[k] = m[(k + 397) % 624] ^ _twist(y)
    return np.array(m, dtype=np.uint32)


def last_word(new_0_622, top_bit=0):
    """Word 623 of a block whose words 0..622 are given: the state has 19937 bits, so of a block's 624 words only 623 (and one bit) are free.  new[623] =
    new[396] ^ twist(old[623] & UPPER | new[0] & LOWER), and `top_bit` is that one free bit (the previous block's word 623)."""
    y = (_UP if top_bit else 0) | (int(new_0_622[0]) & _LO)
    return int(new_0_622[396]) ^ _twist(y)


def mt_backward(new):
    """The block BEFORE `new`: its words 1..623 and the top bit of word 0 are determined; the low 31 bits of word 0 are free for the generator (they
    are never read) and are set here to what makes the returned block itself the image of a block before it (so that the step can be repeated)."""
    n = [int(v) for v in new]
    old = [0] * 624
    y = _untwist(n[623] ^ n[396])
    assert (y & _LO) == (n[0] & _LO), "not the image of any block: word 623 does not fit words 0 and 396 (see last_word)"
    old[623] = y & _UP
    for k in range(622, -1, -1):
        src = n[k - 227] if k >= 227 else old[k + 397]
        y = _untwist(n[k] ^ src)
        old[k] |= y & _UP
        old[k + 1] |= y & _LO
    old[0] |= _untwist(old[623] ^ old[396]) & _LO
    return np.array(old, dtype=np.uint32)


def raw_stream(rng, count):
    """`count` tempered outputs from the state rng = {mti, mt[624]} and the state a sequential consumer is left with after them (numpy's MT19937
    regenerates lazily, like R: a position on a block boundary stays in the old block with mti = 624)."""
    bg = np.random.MT19937()
    bg.state = {"bit_generator": "MT19937", "state": {"key": np.asarray(rng[1:625], dtype=np.uint32).copy(), "pos": int(rng[0])}}
    raw = bg.random_raw(int(count)).astype(np.uint32)
    st = bg.state["state"]
    end = np.empty(625, dtype=np.uint32)
    end[0] = st["pos"]
    end[1:] = st["key"]
    return raw, end


def unif(raw):
    """unif_rand()'s mapping of tempered outputs (fixup into the open interval)."""
    v = np.asarray(raw, dtype=np.float64) * 2.3283064365386963e-10
    half = 0.5 * 2.328306437080797e-10
    v = np.where(v <= 0.0, half, v)
    return np.where(1.0 - v <= 0.0, 1.0 - half, v)


# ---- the serial model -----------------------------------------------------------------------------------------------------------------------------------
def _exp_rand(u, p):
    """exp_rand() starting at stream index p of the uniforms u: (value, positions consumed, smallest |v - q_i| of its comparisons with q)."""
    a, v, k = 0.0, u[p], 1
    while True:
        v += v
        if v > 1.0:
            break
        a += Q[0]
    v -= 1.0
    margin = abs(v - Q[0])
    if v <= Q[0]:
        return a + v, k, margin
    i, umin = 0, u[p + k]
    k += 1
    while True:
        ustar = u[p + k]
        k += 1
        if umin > ustar:
            umin = ustar
        i += 1
        margin = min(margin, abs(v - Q[i])) if i < 15 else margin        # (q[15] = 1.0 ends every search: v <= 1 always)
        if not v > Q[i]:
            break
    return a + umin * Q[0], k, margin


def draw(rng, y, offset, fits):
    """One latent draw of all observations from the generator state rng (625 words).  Returns a dict: x (deviates), lat (new latents, offset removed),
    used (positions per observation), margin and qmargin (per observation), exp (took the exponential branch), exp_len (longest exp_rand), exp_rej (exponential
    proposals rejected), norm_rej (normals rejected), aa, end (generator state after the draw), start (absolute position of every observation)."""
    from stan4bart_amd.rcompat import qnorm
    n = len(y)
    count = 4 * n + 4096
    while True:
        raw, _ = raw_stream(rng, count)
        u = unif(raw)
        z = qnorm((np.floor(BIG * u[:-1]) + u[1:]) / BIG).tolist()
        ul = u.tolist()
        out = _draw_on(ul, z, y, offset, fits, count - 64)
        if out is not None:
            break
        count *= 2
    total = int(out["used"].sum())
    out["end"] = raw_stream(rng, total)[1]
    out["start"] = int(rng[0]) + np.concatenate([[0], np.cumsum(out["used"])[:-1]]).astype(np.int64)
    return out


def _draw_on(u, z, y, offset, fits, limit):
    n = len(y)
    x = np.zeros(n); lat = np.zeros(n); used = np.zeros(n, dtype=np.int64); margin = np.full(n, np.inf); qmargin = np.full(n, np.inf)
    isexp = np.zeros(n, dtype=bool); explen = np.zeros(n, dtype=np.int64); exprej = np.zeros(n, dtype=np.int64); normrej = np.zeros(n, dtype=np.int64)
    aas = np.zeros(n)
    p = 0
    for i in range(n):
        mean = float(fits[i]) + float(offset[i])
        pos = y[i] > 0.0
        lower = 0.0 - mean if pos else mean - 0.0
        p0, mg, qm = p, math.inf, math.inf
        if lower < 0.0:
            while True:
                if p >= limit:
                    return None
                xi = z[p]
                p += 2
                mg = min(mg, abs(xi - lower))
                if not xi < lower:
                    break
                normrej[i] += 1
        else:
            isexp[i] = True
            aa = 0.5 * (lower + math.sqrt(lower * lower + 4.0))
            aas[i] = aa
            while True:
                if p >= limit:
                    return None
                e, k, m = _exp_rand(u, p)
                explen[i] = max(explen[i], k)
                xi = e / aa + lower
                uu = u[p + k]
                p += k + 1
                d = xi - aa
                r = math.exp(-0.5 * d * d)
                mg = min(mg, abs(uu - r))
                qm = min(qm, m)
                if not uu > r:
                    break
                exprej[i] += 1
        zz = mean + xi if pos else mean - xi
        x[i] = xi; lat[i] = zz - float(offset[i]); used[i] = p - p0; margin[i] = mg; qmargin[i] = qm
    return dict(x=x, lat=lat, used=used, margin=margin, qmargin=qmargin, exp=isexp, exp_len=explen, exp_rej=exprej, norm_rej=normrej, aa=aas)


def table_walk(used, lim):
    """How k_latents2 walks these observations, from the positions each consumes alone: chunks of L_CH, batches of at most L_NB; inside a batch
    observation i is resolved from slack o and hands on o + used - 2; an entry above 254 is the sentinel (not taken: the observation opens the next
    batch at slack 0), a taken one of 64 or more ends the batch.  Returns per observation (index in its batch, slack it was resolved from, next-slack it
    handed on) and the number of sentinel stops; an observation that is refused as the FIRST of a batch is outside the kernel's domain (asserted)."""
    n = len(used)
    idx = np.zeros(n, dtype=np.int64); slack = np.zeros(n, dtype=np.int64); nxt = np.zeros(n, dtype=np.int64)
    sentinels = 0
    for c0 in range(0, n, lim["ch"]):
        ch = min(lim["ch"], n - c0)
        done = 0
        while done < ch:
            nb, o, cnt = min(lim["nb"], ch - done), 0, 0
            for i in range(nb):
                g = c0 + done + i
                nx = o + int(used[g]) - 2
                if nx > 254:
                    sentinels += 1
                    assert i > 0, f"observation {g} consumes {int(used[g])} positions from slack 0: outside the kernel's domain"
                    break
                idx[g], slack[g], nxt[g] = i, o, nx
                cnt += 1
                o = nx
                if nx >= 64:
                    break
            done += cnt
    return idx, slack, nxt, sentinels


# ---- crafting a state ----------------------------------------------------------------------------------------------------------------------------------
def craft_state(mti, chosen, seed):
    """A generator state {mti, mt[624]} whose tempered output at absolute stream position g (624 * block + index; the state given is block 0, the next
    draw is position mti) is chosen[g] for every key of `chosen`.  All keys lie in ONE block, at indices 0..622 (block 0: at or after mti).  The other
    words of that block are filler from `seed`; an earlier block is reached by running the generator backwards.  The forward run checks the result."""
    g = np.random.default_rng(seed)
    keys = sorted(chosen)
    b = keys[0] // 624
    assert keys[-1] // 624 == b and all(k % 624 <= 622 for k in keys) and (b > 0 or keys[0] >= mti)
    words = g.integers(0, 1 << 32, size=624, dtype=np.uint64).astype(np.uint32)
    for k in keys:
        words[k % 624] = untemper(np.uint32(chosen[k]))
    if b > 0:
        words[623] = last_word(words, int(g.integers(0, 2)))
        for _ in range(b):
            words = mt_backward(words)
    rng = np.concatenate([[np.uint32(mti)], words]).astype(np.uint32)
    raw, _ = raw_stream(rng, keys[-1] - mti + 1)
    for k in keys:
        assert int(raw[k - mti]) == int(chosen[k]) & 0xFFFFFFFF, (k, hex(int(raw[k - mti])), hex(int(chosen[k])))
    return rng


def _u_word(g, lo, hi):
    """A tempered output whose uniform lies in [lo, hi)."""
    return int(g.uniform(lo, hi) * 4294967296.0) & 0xFFFFFFFF


def normal_run(g, start, rejections):
    """Outputs for an observation with lower = -0.01 that starts at `start`: `rejections` norm_rand() below it (first uniform in [0.05, 0.45): deviate
    below -0.12), then one above (first uniform in [0.55, 0.95)).  The positions of the OTHER parity all hold accepting values, so that a candidate
    read from a wrong position stops early and shows."""
    out = {}
    for k in range(rejections + 1):
        out[start + 2 * k] = _u_word(g, 0.05, 0.45) if k < rejections else _u_word(g, 0.55, 0.95)
        out[start + 2 * k + 1] = _u_word(g, 0.55, 0.95)
    return out


EXP5 = (0xF8000000, 0x40000000, 0x50000000, 0x60000000, 0x01000000)


def exp_front(start):
    """Outputs for an observation with lower = +0.0 (aa = 1) that consumes exactly FIVE positions: exp_rand() of four (u = 0.96875 -> v = 0.9375, between
    q[1] and q[2]: the search draws three more, the smallest 0.25), the value 0.25 log(2), then a uniform of 0.0039 that accepts it."""
    return {start + k: w for k, w in enumerate(EXP5)}


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------------
def _quant(v):
    return np.round(np.asarray(v, dtype=np.float64) * 1048576.0) / 1048576.0


class Case:
    """name; n; y; offset, fits, lat (the state to inject); rng (625 words: mti, mt); claim (what the case says it hits, checked against the model);
    m1, m2 (the model's two consecutive draws)."""

    def __init__(self, name, y, offset, fits, lat, rng, claim=None):
        self.name, self.n = name, len(y)
        self.y = np.asarray(y, dtype=np.float64)
        self.offset, self.fits, self.lat = _quant(offset), _quant(fits), _quant(lat)
        self.rng = np.asarray(rng, dtype=np.uint32)
        self.claim = dict(claim or {})
        self.m1 = draw(self.rng, self.y, self.offset, self.fits)
        self.m2 = draw(self.m1["end"], self.y, self.offset, self.fits)

    def min_margin(self):
        m = min(self.m1["margin"].min(), self.m2["margin"].min())
        if not self.claim.get("exact_q"):
            m = min(m, self.m1["qmargin"].min(), self.m2["qmargin"].min())
        return float(m)

    def max_used(self):
        return int(max(self.m1["used"].max(), self.m2["used"].max()))

    def __repr__(self):
        return self.name


def _seed_rng(g, mti):
    words = g.integers(0, 1 << 32, size=624, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([[np.uint32(mti)], words]).astype(np.uint32)


def _means(g, kind, n):
    """(y, offset, fits): 'normal' — means N(0, 1.5^2), y drawn from the probit model; 'wide' — a uniform offset on [-8, 8], y independent of it."""
    if kind == "normal":
        fits = 1.5 * g.standard_normal(n)
        off = 0.25 * g.standard_normal(n)
        y = (fits + off + g.standard_normal(n) > 0.0).astype(np.float64)
    else:
        off = g.uniform(-8.0, 8.0, n)
        fits = 0.25 * g.standard_normal(n)
        y = (g.random(n) < 0.5).astype(np.float64)
    return y, off, fits


def _retry(make, what):
    """make(attempt) -> Case, re-drawn (another seed for a random case, other filler words for a crafted one) until the margin condition holds."""
    for attempt in range(64):
        c = make(attempt)
        if c.min_margin() >= MIN_MARGIN:
            assert c.max_used() <= MAX_POSITIONS, (c.name, c.max_used())
            return c
    raise AssertionError(f"no draw of case {what} keeps every decision {MIN_MARGIN} away from a tie")


def random_case(name, n, kind, mti, seed):
    def make(attempt):
        g = np.random.default_rng([seed, attempt, n])
        y, off, fits = _means(g, kind, n)
        return Case(name, y, off, fits, g.standard_normal(n) - off, _seed_rng(g, mti), dict(n=n, mti=mti))
    return _retry(make, name)


def _filler_obs(n):
    """Observations with lower = -40 (mean 40, y = 1): each accepts its first normal whatever the stream holds (no deviate of norm_rand() is below
    -8.9) and consumes exactly two positions."""
    return np.ones(n), np.zeros(n), np.full(n, 40.0)


def run_case(name, n, obs, rejections, mti, front=False, seed=0):
    """`rejections` rejected normals for observation `obs` (lower = -0.01), every other observation a two-position filler, so that `obs` starts at
    mti + 2 obs exactly; with `front`, observation obs - 1 is a five-position exponential one (lower = +0.0) and `obs` starts at an odd slack."""
    def make(attempt):
        g = np.random.default_rng([seed, attempt, obs, rejections])
        y, off, fits = _filler_obs(n)
        fits[obs] = 0.01
        start = mti + 2 * obs
        chosen = {}
        if front:
            fits[obs - 1] = 0.0
            chosen.update(exp_front(start - 2))
            start += 3
        chosen.update(normal_run(g, start, rejections))
        rng = craft_state(mti, chosen, int(g.integers(1 << 30)))
        return Case(name, y, off, fits, g.standard_normal(n), rng,
                    dict(obs=obs, rejections=rejections, used=2 * (rejections + 1), start=start, front=front))
    return _retry(make, name)


def exp_case(name, words, mti=5, n=8, obs=0, lower=0.0, claim=None, seed=0):
    """Observation `obs` takes the exponential branch (mean = -lower, y = 1) and reads `words` from its first position on; fillers elsewhere."""
    def make(attempt):
        g = np.random.default_rng([seed, attempt, len(words)])
        y, off, fits = _filler_obs(n)
        fits[obs] = -lower
        start = mti + 2 * obs
        chosen = {start + k: w for k, w in enumerate(words) if w is not None}
        rng = craft_state(mti, chosen, int(g.integers(1 << 30)))
        return Case(name, y, off, fits, g.standard_normal(n), rng, dict(obs=obs, start=start, **(claim or {})))
    return _retry(make, name)


def boundary_cases(count=3):
    """Draws that END exactly on a block boundary (hand-back: mti = 624 with the OLD block), found by scanning n with the model; one has n > L_CH."""
    out = []
    g = np.random.default_rng(4242)
    nmax = 2600
    y, off, fits = _means(g, "normal", nmax)
    lat = g.standard_normal(nmax)
    for mti, lo in ((17, 100), (400, 600), (3, 2049)):
        for attempt in range(64):
            rng = _seed_rng(np.random.default_rng([77, mti, attempt]), mti)
            m = draw(rng, y, off, fits)
            ends = mti + np.cumsum(m["used"])
            hit = [int(k) + 1 for k in np.nonzero(ends % 624 == 0)[0] if k + 1 >= lo]
            ok = None
            for n in hit:
                c = Case(f"boundary-n{n}-mti{mti}", y[:n], off[:n], fits[:n], lat[:n], rng, dict(end_mti=624, n=n))
                if c.min_margin() >= MIN_MARGIN:
                    ok = c
                    break
            if ok is not None:
                out.append(ok)
                break
        else:
            raise AssertionError("no block-boundary ending found")
    assert len(out) >= count
    return out


def over_limit_case():
    """OUTSIDE the kernel's domain, never part of cases(): 128 rejected normals for the first observation (258 positions from slack 0).  The oracle and
    the emulated layer go on drawing; k_latents2 must end with S4B_ERR_INTERNAL.  Built without the domain assertion of _retry."""
    g = np.random.default_rng(128)
    n = 40
    y, off, fits = _filler_obs(n)
    fits[0] = 0.01
    rng = craft_state(2, normal_run(g, 2, 128), 128)
    return Case("over-limit-r128", y, off, fits, g.standard_normal(n), rng, dict(obs=0, rejections=128, used=258))


_CASES = {}


def cases(big=False):
    """All cases (built once per process).  `big` adds the n = 100 000 case of the GPU file (ring wraps under wide tails)."""
    key = bool(big)
    if key in _CASES:
        return _CASES[key]
    lim = kernel_limits()
    nb, ch = lim["nb"], lim["ch"]
    out = []
    # (5) x (4): batch, wave and chunk edges; both mean laws; every start position with both laws
    for i, n in enumerate(SIZES):
        for k, kind in enumerate(("normal", "wide")):
            mti = START_MTI[(i + 2 * k + i // 4) % 4]
            out.append(random_case(f"size-n{n}-{kind}-mti{mti}", n, kind, mti, seed=1000 + 2 * i + k))
    out += boundary_cases()
    # crafted runs of rejected normals: either side of the two-ballot window (32 candidates), next-slack either side of 64, the last representable
    for place in (0, nb // 2, nb - 1):
        for r in (31, 32, 33):
            out.append(run_case(f"run-r{r}-place{place}", 3 * nb, nb + place, r, mti=3 + (place & 1), seed=1))
        for r in (126, 127):
            out.append(run_case(f"run-r{r}-place{place}", 3 * nb, place, r, mti=2 + (place & 1), seed=2))
    for place in (nb // 2, nb - 1):
        for r in (30, 31):                  # next-slack 63 and 65: an odd slack needs a five-position exponential observation in front
            out.append(run_case(f"run-odd-r{r}-place{place}", 3 * nb, nb + place, r, mti=4, front=True, seed=3))
    for r in (126, 127):                    # 3 + 2 r >= 255: the sentinel; the observation opens the next batch at slack 0
        out.append(run_case(f"run-sentinel-r{r}", 3 * nb, nb // 2, r, mti=6, front=True, seed=4))
    for obs in (ch - 1, ch):                # the chunk edge, six blocks in: the chosen block is reached by running the generator backwards
        for r in (32, 127):
            out.append(run_case(f"run-chunk-r{r}-obs{obs}", ch + 52, obs, r, mti=7, seed=5))
    # crafted exponential branch
    out.append(exp_case("exp-17-positions", [0x80000000] + [None] * 16 + [0x01000000], claim=dict(exp_len=17, used=18, exact_q=True)))
    out.append(exp_case("exp-first-ffffffff", [0xFFFFFFFF], claim=dict(first=0xFFFFFFFF, exp_len=12, exact_q=True)))
    out.append(exp_case("exp-first-00000000", [0x00000000], claim=dict(first=0)))
    out.append(exp_case("exp-3-rejections", [3, 0x90000000, 5, 0xA0000000, 6, 0xB0000000, 0xC0000000, 0x10000000], claim=dict(exp_rej=3, used=8)))
    # a 17-position exp_rand() across the end of a block, and across the end of the range the first refill generates (three blocks: E / EL end
    # L_EMAX positions before it, the rest waits for the next block)
    out.append(exp_case("exp-17-block-end", [0x80000000], mti=4, n=320, obs=305, claim=dict(exp_len=17, crosses=624, exact_q=True)))
    for start in (3 * 624 - lim["emax"] - 10, 3 * 624 - lim["emax"] + 1):
        out.append(exp_case(f"exp-17-range-end-{start}", [0x80000000] + [None] * 16 + [0x01000000], mti=4 + (start & 1), n=960, obs=(start - 4) // 2,
                            claim=dict(exp_len=17, used=18, exact_q=True, range_end=3 * 624 - lim["emax"])))
    out.append(_zero_case())
    out.append(_far_case())
    out.append(_convention_case())
    if big:
        out.append(random_case("big-n100000-wide", 100000, "wide", 311, seed=9))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    _CASES[key] = out
    return out


def _zero_case():
    """lower = +-0.0: mean = +0.0 and -0.0 with either y (latent = fits = offset = -0.0 is the one way to a mean of -0.0 through the stored
    conventions); all four take the exponential branch with aa = 1."""
    def make(attempt):
        g = np.random.default_rng([11, attempt])
        n = 8
        y, off, fits = _filler_obs(n)
        lat = g.standard_normal(n)
        y[:4] = (1.0, 0.0, 1.0, 0.0)
        fits[:4] = (0.0, 0.0, -0.0, -0.0); off[:4] = (0.0, 0.0, -0.0, -0.0); lat[:4] = (0.0, 0.0, -0.0, -0.0)
        c = Case("exp-lower-zero", y, off, fits, lat, _seed_rng(g, 9), dict(exp_obs=[0, 1, 2, 3], aa=1.0))
        assert np.signbit(c.fits[2:4]).all() and np.signbit(c.offset[2:4]).all() and np.signbit(c.lat[2:4]).all()      # (rounding to the grid keeps the sign)
        return c
    return _retry(make, "exp-lower-zero")


def _far_case():
    """lower = 8 and 40 (both signs of y): the exponential branch far out, aa ~ lower."""
    def make(attempt):
        g = np.random.default_rng([12, attempt])
        n = 12
        y, off, fits = _filler_obs(n)
        y[:4] = (1.0, 0.0, 1.0, 0.0)
        fits[:4] = (-8.0, 8.0, -40.0, 40.0)
        return Case("exp-lower-8-40", y, off, fits, g.standard_normal(n), _seed_rng(g, 10), dict(exp_obs=[0, 1, 2, 3], lowers=[8.0, 8.0, 40.0, 40.0]))
    return _retry(make, "exp-lower-8-40")


def _convention_case():
    """Offsets of order 1e3 under means of order 1, previous latents unrelated to either: latent - residual, + offset, - offset do not cancel."""
    def make(attempt):
        g = np.random.default_rng([13, attempt])
        n = 100
        off = 1e3 * g.standard_normal(n)
        mean = 1.5 * g.standard_normal(n)
        y = (mean + g.standard_normal(n) > 0.0).astype(np.float64)
        return Case("conventions-offset-1e3", y, off, _quant(mean) - _quant(off), 30.0 * g.standard_normal(n), _seed_rng(g, 100), dict(offset_scale=1e3))
    return _retry(make, "conventions-offset-1e3")


# ---- running a case through a library -------------------------------------------------------------------------------------------------------------------
def sampler_args(case):
    """A small probit sampler with the case's response (the response is fixed at creation; everything else of the case goes in through set_state)."""
    from stan4bart_amd import make_sampler_args
    g = np.random.default_rng(5)
    xb = np.asfortranarray(g.random((case.n, 2)))
    X = g.random((case.n, 1))
    return make_sampler_args(case.y, xb, X=X, family="binomial", iter=4, warmup=2, bart_args={"n.trees": 2})


def inject(sampler, case, StateView):
    """The case's state into a sampler: r_rng, offset, total_fits, latents of its own state blob replaced."""
    sv = StateView(sampler.get_state())
    assert sv.binary and sv.n == case.n
    sv.set("r_rng", np.concatenate([case.rng, [np.uint32(0)]]).astype(np.uint32))
    sv.set("offset", case.offset); sv.set("total_fits", case.fits); sv.set("latents", case.lat)
    sampler.set_state(sv.bytes())
    return sv
