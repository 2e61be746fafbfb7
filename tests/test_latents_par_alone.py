"""The model, cases and geometry of tests/latent_par_cases.py where no GPU is needed (k_latents_par alone on the MI355X: tests/test_gpu_latents_par_alone.py):
the numpy Philox against Random123's known answers and against the header compiled for the host on counters with a single word set; every case's
model against philox_trunc_normal of csrc/philox.hpp compiled with g++ — values within the bound evaluated for glibc; the header reports no attempt
count, so "same attempt, same deviate" is INFERRED: the host program names the candidate nearest to the header's x among all attempts up to two past
the model's —; every case's claims (attempt and branch counts, no undecided decision); the long-double model against mpmath at 40 digits; the draw
that is refused (a mean whose square overflows); the launch geometry as a hand-written table against what the module reads out of dev_hip.hip."""
import os
import struct
import subprocess

import mpmath as mp
import numpy as np
import pytest

import latent_par_cases as P
from test_latents_parallel import KAT, _compile


HOST = """
#include "philox.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
// in: k0, k1, draw index, n, lower[n], the model's attempt[n] (1-based) and accepted deviate[n] (0 z0, 1 z1, 2 exponential proposal)
// out per observation: x, accepted (0 / 1), and the attempt and deviate whose candidate — formed here from the header's own generator and uniforms —
// is nearest to x among all attempts up to two past the model's (the model's own on a tie).  The header inlined into its loop and this restatement
// need not agree bit for bit (the compiler may fuse sin and cos into one sincos there), hence nearest and not equal.
static double cand_of(const uint32_t* k, uint64_t draw, uint32_t i, int t, int dev, double l) {
  const s4b::Philox4 c = {{(uint32_t)draw, (uint32_t)(draw >> 32), i, (uint32_t)t}};
  const s4b::Philox4 r = s4b::philox4x32_10(c, k[0], k[1]);
  const double u1 = s4b::philox_u53(r.v[0], r.v[1]), u2 = s4b::philox_u53(r.v[2], r.v[3]);
  if (dev == 2) { const double lam = 0.5 * (l + sqrt(l * l + 4.0)); return l - log(u1) / lam; }
  const double rad = sqrt(-2.0 * log(u1)), th = 6.283185307179586 * u2;
  return dev == 0 ? rad * cos(th) : rad * sin(th);
}
int main() {
  uint32_t k[2]; uint64_t draw; int64_t n;
  if (fread(k, 4, 2, stdin) != 2 || fread(&draw, 8, 1, stdin) != 1 || fread(&n, 8, 1, stdin) != 1) return 2;
  std::vector<double> lo((size_t)n); std::vector<int32_t> att((size_t)n), dev((size_t)n);
  if (fread(lo.data(), 8, (size_t)n, stdin) != (size_t)n || fread(att.data(), 4, (size_t)n, stdin) != (size_t)n || fread(dev.data(), 4, (size_t)n, stdin) != (size_t)n) return 2;
  for (int64_t i = 0; i < n; ++i) {
    const double l = lo[(size_t)i];
    double x; const bool ok = s4b::philox_trunc_normal(k[0], k[1], draw, (uint32_t)i, l, x);
    int bt = att[(size_t)i] - 1, bd = dev[(size_t)i];
    double best = fabs(cand_of(k, draw, (uint32_t)i, bt, bd, l) - x);
    for (int t = 0; t <= att[(size_t)i] + 1; ++t)
      for (int d = (l < 0.0 ? 0 : 2); d <= (l < 0.0 ? 1 : 2); ++d) {
        const double e = fabs(cand_of(k, draw, (uint32_t)i, t, d, l) - x);
        if (e < best) { best = e; bt = t; bd = d; }
      }
    const double rec[4] = {x, ok ? 1.0 : 0.0, (double)(bt + 1), (double)bd};
    fwrite(rec, 8, 4, stdout);
  }
}
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("latpar"), HOST, "latpar")


def _host_draw(exe, key, index, lower, attempts, branch):
    n = len(lower)
    msg = struct.pack("<IIQq", key & 0xFFFFFFFF, key >> 32, index, n) + np.asarray(lower, dtype=np.float64).tobytes() + \
        np.asarray(attempts, dtype=np.int32).tobytes() + np.asarray(branch, dtype=np.int32).tobytes()
    out = subprocess.run([exe], input=msg, stdout=subprocess.PIPE, check=True).stdout
    return np.frombuffer(out, dtype=np.float64).reshape(n, 4)


# ---- the generator -----------------------------------------------------------------------------------------------------------------------------------------
def test_numpy_philox_known_answers():
    for ctr, key, want in KAT:
        assert tuple(int(v) for v in P.philox4x32_10(*ctr, *key)) == want, (ctr, key)
    c = np.array([k[0] for k in KAT], dtype=np.uint64)          # (vectorised over counters under one key)
    got = P.philox4x32_10(c[:, 0], c[:, 1], c[:, 2], c[:, 3], *KAT[0][1])
    assert tuple(int(v[0]) for v in got) == KAT[0][2]


def test_numpy_philox_on_single_word_counters(tmp_path):
    """A counter with only the attempt word set, one with only the observation word, one with only each half of the draw index, under a key with
    different halves: against the header compiled for the host (no published vector has such a counter)."""
    exe = _compile(tmp_path, """
#include "philox.hpp"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
  s4b::Philox4 c; for (int i = 0; i < 4; ++i) c.v[i] = (uint32_t)strtoul(argv[1 + i], nullptr, 0);
  const s4b::Philox4 r = s4b::philox4x32_10(c, (uint32_t)strtoul(argv[5], nullptr, 0), (uint32_t)strtoul(argv[6], nullptr, 0));
  printf("%u %u %u %u\\n", r.v[0], r.v[1], r.v[2], r.v[3]);
}
""", "kat1")
    key = (0x01234567, 0x89ABCDEF)
    seen = set()
    for ctr in ((0, 0, 0, 4095), (0, 0, 0x00010001, 0), (5, 0, 0, 0), (0, 5, 0, 0), (0, 0, 0, 0)):
        out = subprocess.run([exe, *map(str, ctr), *map(str, key)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
        got = tuple(int(v) for v in P.philox4x32_10(*ctr, *key))
        assert got == tuple(int(v) for v in out), ctr
        seen.add(got)
    assert len(seen) == 5
    assert tuple(int(v) for v in P.philox4x32_10(0, 0, 0, 0, key[1], key[0])) not in seen, "the key halves are interchangeable"


def test_uniform_is_the_cell_midpoint_in_double():
    one = np.array([1], dtype=np.uint64)
    assert P.u53(0 * one, 0 * one)[0] == 2.0 ** -54
    assert P.u53(one, 2047 * one)[0] == (2.0 ** 21 + 0.5) * 2.0 ** -53                    # (the low 11 bits of the second word are dropped)
    assert P.u53(one, 2048 * one)[0] == (2.0 ** 21 + 1.5) * 2.0 ** -53
    assert P.u53(0xFFFFFFFF * one, 0xFFFFFFFF * one)[0] == 1.0                            # (2^53 - 1/2 is no double: the last cell rounds to 1, log(1) = 0)


# ---- the model against the header on the host --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_model_matches_the_header_on_the_host(host, name):
    case = P.case(name)
    key = case.key_value()
    for k, m in enumerate((case.m1, case.m2)):
        out = _host_draw(host, key, (case.index + k) & ((1 << 64) - 1), m["lower"], m["attempts"], m["branch"])
        assert np.all(out[:, 1] == 1.0)
        bad = np.nonzero((out[:, 2] != m["attempts"]) | (out[:, 3] != m["branch"]))[0]
        assert bad.size == 0, f"{case.name}, draw {k}: the header accepted another candidate than the model for {bad.size} observations, first {bad[0]} " \
                              f"(model: attempt {m['attempts'][bad[0]]}, deviate {m['branch'][bad[0]]}; header: {out[bad[0], 2:]}; lower {m['lower'][bad[0]]!r})"
        d = np.abs(out[:, 0].astype(P.LD) - m["x"]).astype(np.float64)
        b = P.BOUND_FACTOR * m["bound"]["glibc"]
        worst = int(np.argmax(d - b))
        assert np.all(d <= b), f"{case.name}, draw {k}: observation {worst}: {out[worst, 0]!r} against {m['x'][worst]!r}, bound {b[worst]:.3g}"
        assert np.all(out[:, 0] >= m["lower"])


def test_a_mean_whose_square_overflows_is_refused_on_the_host(host):
    """y = 0, mean 1e200: lam = inf, no proposal in 4 096 attempts, the header returns false and x = lower (what the kernel turns into S4B_ERR_I_LATENT).
    The largest bound inside the domain draws."""
    out = _host_draw(host, 7, 0, [P.failure_lower(), 1.3e154], [1, 1], [2, 2])
    assert out[0, 1] == 0.0 and out[0, 0] == P.failure_lower()
    assert out[1, 1] == 1.0 and out[1, 0] >= 1.3e154


# ---- the cases' claims ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_case_claims(name):
    case = P.case(name)
    assert case.undecided() == 0
    got = (case.counts(case.m1), case.counts(case.m2))
    assert got == P.CLAIMS[case.name], (case.name, got)
    if case.n >= 256:
        assert min(got[0]) >= 1 and min(got[1]) >= 1, (case.name, got)
    for m in (case.m1, case.m2):
        assert np.all(m["branch"] >= 0) and np.all(m["attempts"] >= 1)
        assert np.array_equal(m["branch"] == 2, ~(m["lower"] < 0.0))
        assert np.all(m["x"] >= m["lower"])
        assert np.all(np.isfinite(m["bound"]["device"])) and np.all(m["bound"]["device"] >= m["bound"]["glibc"])
    assert case.index + 1 == (case.index + 1) & ((1 << 64) - 1), "a draw index that wraps is not a case"


def test_the_cases_cover_what_they_are_there_for():
    CASES = P.cases()
    by = {c.name: c for c in CASES}
    assert {c.index for c in CASES} >= {0, 1, (1 << 32) - 1, 1 << 32, (1 << 63) + 5}
    keys = [c.key for c in CASES if c.key != P.OWN_KEY]
    assert any(k & 0xFFFFFFFF == 0 and k >> 32 for k in keys) and any(k >> 32 == 0 and k for k in keys) and (1 << 64) - 1 in keys
    assert sum(c.key == P.OWN_KEY for c in CASES) == 2
    assert {c.n for c in CASES} >= {1, 255, 256, 257, 1000, 1024, 1025, 65537, 262147, 1048577}
    assert np.all(by["n255-key-low0-draw1-ones"].y == 1.0) and np.all(by["n256-key-high0-draw-2p32m1-zeros"].y == 0.0)
    a = by[P.TRIPLE[0]]
    for name in P.TRIPLE[1:]:
        b = by[name]
        assert (b.key, b.index) == (a.key, a.index)
        for f in ("y", "offset", "fits", "lat"):
            assert np.array_equal(getattr(b, f)[:1000], getattr(a, f))
        for ma, mb in ((a.m1, b.m1), (a.m2, b.m2)):          # the model itself is independent of n
            assert np.array_equal(mb["x"][:1000], ma["x"]) and np.array_equal(mb["attempts"][:1000], ma["attempts"])
    m = by["n65537-shared"].m1
    assert (m["attempts"][65536:] >= 1).all() and int((m["attempts"][256:] >= 2).sum()) > 0          # (rejections beyond the first trip and beyond 16 bits)
    cv = by["conventions-offset-1e3"]
    assert np.abs(cv.offset).max() > 1e3 and np.abs(cv.m1["mean"]).max() < 10.0


def test_the_long_double_model_against_mpmath():
    """A few dozen observations per case at 40 digits: same attempt, same deviate, and the long-double value within 2^-11 of the bound derived for
    doubles (the bound is linear in the unit roundoff; the model's is 2^-64 against 2^-53): the reference's own error is far inside the allowance."""
    for case in P.cases():
        key = case.key_value()
        for k, m in enumerate((case.m1, case.m2)):
            order = np.argsort(-m["attempts"], kind="stable")
            pick = sorted(set(order[:12].tolist()) | set(np.nonzero(m["branch"] == 1)[0][:6].tolist()) | set(range(min(case.n, 24 if case.n <= 24 else 6)))
                          | set(np.random.default_rng(case.n).integers(0, case.n, 8).tolist()))
            for i in pick:
                x, att, dev = P.mp_draw(key, case.index + k, i, m["lower"][i])
                assert (att, dev) == (m["attempts"][i], m["branch"][i]), (case.name, k, i)
                with mp.workdps(40):
                    err = float(abs(x - mp.mpf(int(np.frexp(m["x"][i])[0] * P.LD(2.0) ** 64)) * mp.mpf(2) ** (int(np.frexp(m["x"][i])[1]) - 64)))
                assert err <= m["bound"]["device"][i] * 2.0 ** -11, (case.name, k, i, err, m["bound"]["device"][i])


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------------------------
def _check_table(lim):
    for n in sorted(set(P.CASE_N.values())):
        assert P.geometry(n, lim) == P.GEOMETRY[n], (n, P.geometry(n, lim), P.GEOMETRY[n])


def test_geometry_table():
    lim = P.kernel_geometry()
    assert lim == dict(block=256, cap=1024)
    _check_table(lim)
    g = {n: P.geometry(n, lim) for n in P.GEOMETRY}
    assert g[256][1] == 1 and g[257][1] == 2                       # the second trip starts at observation 256
    assert g[1024][0] == 1 and g[1025][0] == 2                     # one / two workgroups
    assert g[1048577] == (1024, 5, 1) and (1048577 + 3) // 4 > 1024 * 256          # the cap, a ragged fifth trip


@pytest.mark.parametrize("old, new", [("constexpr int BLOCK = 256;", "constexpr int BLOCK = 128;"),
                                      ("a.grid = (int)std::min<int64_t>(1024,", "a.grid = (int)std::min<int64_t>(512,")], ids=["BLOCK-128", "cap-512"])
def test_geometry_table_fails_on_an_edited_constant(tmp_path, old, new):
    src = open(os.path.join(P.CSRC, "dev_hip.hip")).read()
    assert src.count(old) == 1
    f = tmp_path / "dev_hip.hip"
    f.write_text(src.replace(old, new))
    lim = P.kernel_geometry(src_path=str(f))          # (outside the block below: only the table may fail)
    assert lim != dict(block=256, cap=1024)
    with pytest.raises(AssertionError):
        _check_table(lim)


def test_key_hash_is_a_function_of_seed_and_state():
    a, b = P.sampler_key(12345), P.sampler_key(999)
    assert a != b and a == P.sampler_key(12345) and 0 < a < 1 << 64
    st = np.zeros(625, dtype=np.uint32)
    assert P.latent_key(st, 0) != P.latent_key(st, 1)
    st2 = st.copy(); st2[624] = 1
    assert P.latent_key(st, 0) != P.latent_key(st2, 0)
