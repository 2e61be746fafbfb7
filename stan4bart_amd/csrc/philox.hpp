// Philox4x32-10 (Salmon, Moraes, Dror & Shaw 2011, "Parallel random numbers: as easy as 1, 2, 3") and the exact
// lower-truncated standard normal of the parallel probit latents (latent mode 1).
//
// Counter-based: the output is a pure function of (counter, key), so every observation of a latent draw takes its
// random numbers without a shared stream.  Counter = {draw index low, draw index high, observation, attempt}, key = 64
// bits per chain: no counter repeats within a chain (an observation gives up after TN_MAX_ATTEMPTS < 2^32 attempts).
//
// Plain C++ on the host (the known-answer test compiles this header with g++), __host__ __device__ under hipcc.
#ifndef S4B_PHILOX_HPP
#define S4B_PHILOX_HPP

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define S4B_PHX __host__ __device__ inline
#else
#define S4B_PHX inline
#endif

namespace s4b {

struct Philox4 { uint32_t v[4]; };

S4B_PHX void philox_mulhilo(uint32_t a, uint32_t b, uint32_t& hi, uint32_t& lo) {
  const uint64_t p = (uint64_t)a * (uint64_t)b;
  hi = (uint32_t)(p >> 32); lo = (uint32_t)p;
}
// ten rounds, the key bumped by the Weyl constants between rounds (Random123's philox4x32_R with R = 10)
S4B_PHX Philox4 philox4x32_10(Philox4 c, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    uint32_t hi0, lo0, hi1, lo1;
    philox_mulhilo(0xD2511F53u, c.v[0], hi0, lo0);
    philox_mulhilo(0xCD9E8D57u, c.v[2], hi1, lo1);
    const Philox4 o = {{hi1 ^ c.v[1] ^ k0, lo1, hi0 ^ c.v[3] ^ k1, lo0}};
    c = o;
  }
  return c;
}
// a uniform on (0, 1] from two words: 53 bits m, (m + 1/2) 2^-53 formed in double — the midpoint of its cell below m = 2^52, rounded to even from
// there on (the sum needs 54 bits), so never 0, and 1 for the one value m = 2^53 - 1 (log(1) = 0: rad = 0 or z = lower, both harmless) —, so that
// -log(u) reaches 37.4 and the tails are not cut at 32-bit resolution
S4B_PHX double philox_u53(uint32_t hi, uint32_t lo) {
  const uint64_t m = ((uint64_t)hi << 21) ^ (uint64_t)(lo >> 11);
  return ((double)m + 0.5) * 1.1102230246251565e-16;   // 2^-53
}

// every attempt is accepted with probability >= 0.75 while lower^2 is finite: 4 096 failures in a row only happen to a bound that is not finite
// or whose square overflows (|lower| above sqrt(DBL_MAX), about 1.3e154: lam = inf and the acceptance probability is 0)
constexpr int TN_MAX_ATTEMPTS = 1 << 12;
// x ~ N(0, 1) | x >= lower, exactly, from the counters {draw, obs, attempt = 0, 1, ...}; one Philox block (two uniforms) per attempt.
//   lower < 0:  normal rejection — the two Box-Muller deviates of the block are proposed in turn (acceptance >= 1 - 0.5^2 per attempt);
//   lower >= 0: Robert's (1995) exponential proposal x = lower + E / lam, lam = (lower + sqrt(lower^2 + 4)) / 2, accepted with
//               probability exp(-(x - lam)^2 / 2) (acceptance >= 0.76 per attempt, -> 1 as lower grows).
// The switch at 0 is where the two cost about the same per accepted draw (and where dbarts switches).  Returns false (x = lower) when no
// attempt was accepted: only a bound that is not finite, or beyond about 1.3e154 on the exponential branch, gets there.
S4B_PHX bool philox_trunc_normal(uint32_t k0, uint32_t k1, uint64_t draw, uint32_t obs, double lower, double& x) {
  Philox4 c = {{(uint32_t)draw, (uint32_t)(draw >> 32), obs, 0u}};
  if (lower < 0.0) {
    for (int t = 0; t < TN_MAX_ATTEMPTS; ++t) {
      c.v[3] = (uint32_t)t;
      const Philox4 r = philox4x32_10(c, k0, k1);
      const double u1 = philox_u53(r.v[0], r.v[1]), u2 = philox_u53(r.v[2], r.v[3]);
      const double rad = sqrt(-2.0 * log(u1)), th = 6.283185307179586 * u2;
      const double z0 = rad * cos(th);
      if (z0 >= lower) { x = z0; return true; }
      const double z1 = rad * sin(th);
      if (z1 >= lower) { x = z1; return true; }
    }
  } else {
    const double lam = 0.5 * (lower + sqrt(lower * lower + 4.0));
    for (int t = 0; t < TN_MAX_ATTEMPTS; ++t) {
      c.v[3] = (uint32_t)t;
      const Philox4 r = philox4x32_10(c, k0, k1);
      const double u1 = philox_u53(r.v[0], r.v[1]), u2 = philox_u53(r.v[2], r.v[3]);
      const double z = lower - log(u1) / lam, d = z - lam;
      if (u2 <= exp(-0.5 * d * d)) { x = z; return true; }
    }
  }
  x = lower;
  return false;
}

// The standard normal deviate of element (row, draw) of a posterior predictive read-out (s4b_predict_ppd): the cosine deviate of
// Box-Muller from the two uniforms of ONE block, counter = {row low, row high, draw, PPD_TAG}.  A pure function of (key, row, draw).  The last
// counter word of the latents above is an attempt number below TN_MAX_ATTEMPTS; PPD_TAG lies above it ("PPD1"), so no block is shared with them
// even under the same key.  The sine deviate of the block is not used.
constexpr uint32_t PPD_TAG = 0x50504431u;
static_assert(PPD_TAG >= (uint32_t)TN_MAX_ATTEMPTS, "the tag must differ from every attempt number of philox_trunc_normal");
S4B_PHX double philox_normal(uint32_t k0, uint32_t k1, uint64_t row, uint32_t draw) {
  const Philox4 c = {{(uint32_t)row, (uint32_t)(row >> 32), draw, PPD_TAG}};
  const Philox4 r = philox4x32_10(c, k0, k1);
  const double u1 = philox_u53(r.v[0], r.v[1]), u2 = philox_u53(r.v[2], r.v[3]);
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}
// The (0, 1] uniform of element (row, draw) of a posterior predictive check with a binary response (s4b_predict_check): philox_u53 of
// the FIRST TWO words of philox_normal's block, the same counter and key (u1 there).  A pure function of (key, row, draw).
S4B_PHX double philox_uniform(uint32_t k0, uint32_t k1, uint64_t row, uint32_t draw) {
  const Philox4 c = {{(uint32_t)row, (uint32_t)(row >> 32), draw, PPD_TAG}};
  const Philox4 r = philox4x32_10(c, k0, k1);
  return philox_u53(r.v[0], r.v[1]);
}

}  // namespace s4b

#endif
