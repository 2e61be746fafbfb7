// Shared by both translation units of libs4b.so: what the fused tree update (k_step, dev_step.inc) and the persistent sweep (k_sweep,
// dev_sweep.inc) have in common — the workgroup size, the fixed-point exchange words, the proposal images, the written-through
// residual store, the scratch-set header and the hand-over between the main arrays and the scratch sets.
#ifndef S4B_DEV_STEP_SHARED_HPP
#define S4B_DEV_STEP_SHARED_HPP

#include "dev_control.hpp"

namespace s4b {

constexpr int FBLOCK = 512;          // 8 waves: decider, 2 image waves, 5 reducer / loader waves; all 8 run the pass

// ---- exchange of the persistent sweep (dev_sweep.inc): the per-workgroup partial (sum, count) of every bin is ADDED into one of
// XC_COPIES copies of two 64-bit words per bin with agent-scope integer atomics that return nothing — order-free, hence
// deterministic, and a reader fetches XC_COPIES * 2 nb words instead of one partial per workgroup and bin:
//   word 0: [arrivals : 6][ rint(s * 2^24) + 2^52                               : 58]
//   word 1: [arrivals : 6][count : 21][ rint((s - rint(s 2^24) 2^-24) * 2^55) + 2^31 : 37]
// |s| < 2^27 (checked; the partial residuals of a rescaled response are O(1): DESIGN.md 5.0), at most 32 workgroups per copy, fewer than
// 2^16 observations per workgroup (at most 4 096 with the residual in registers; the streaming pass: dev_hip.hip, streamCountOk), so at most
// 2^21 - 1 per copy: no field can carry into its neighbour.  Resolution 2^-55 absolute per partial (observation weights: relative to a bin's
// sums, 2^-55 * max / min weight, at most 2^-25 — dev_hip.hip, wRangeOk).
constexpr int XC_COPIES = 8, XC_WORDS = 128, XC_RING = 4;      // copies; words per copy (2 per bin, 64 bins); ring of exchange buffers
constexpr int XC_BUF_WORDS = XC_COPIES * XC_WORDS;
// (two rings side by side: buffers 0 .. XC_RING-1 take what a step publishes first — speculatively, before its verdict, in the persistent
// sweep —, buffers XC_RING .. 2 XC_RING-1 the statistics a step publishes AGAIN when the verdict did not bear its speculation out)
constexpr int XC_RING_WORDS = 2 * XC_RING * XC_BUF_WORDS;
__device__ __forceinline__ void xc_publish(unsigned long long* cur, int bin, double s, int c, int32_t* errFlag) {
  const double h = rint(s * 16777216.0);
  const double r = s - h * (1.0 / 16777216.0);                  // exact
  if (!(fabs(s) < 134217728.0)) *errFlag |= S4B_ERR_INTERNAL | S4B_ERR_I_RANGE;   // (also NaN) outside the fixed-point range: the chain is invalid
  const long long hi = (long long)h, lo = (long long)rint(r * 36028797018963968.0);
  const unsigned long long w0 = (unsigned long long)(hi + (1ll << 52)) + (1ull << 58);
  const unsigned long long w1 = (unsigned long long)(lo + (1ll << 31)) + ((unsigned long long)(unsigned)c << 37) + (1ull << 58);
  unsigned long long* p = cur + (size_t)(blockIdx.x % XC_COPIES) * XC_WORDS + 2 * bin;
  __hip_atomic_fetch_add(p, w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_add(p + 1, w1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// bytes of one proposal image (see CandSet) and its parts
__host__ __device__ static inline size_t cand_bytes(int nc) {
  size_t b = ((size_t)SF_COUNT * nc * 2 + 15) / 16 * 16 + ((size_t)nc + 15) / 16 * 16 + 128 + (size_t)nc * 8 + ((size_t)nc * 4 + 15) / 16 * 16 +
             (sizeof(MTState) + 15) / 16 * 16 + 16;
  return (b + 255) / 256 * 256;
}
__device__ __forceinline__ CandSet cand_view(const BartArrays& a, int parity, int c) {
  unsigned char* base = a.candBase + (size_t)(2 * parity + c) * (size_t)a.candStride;
  const int nc = a.nc;
  CandSet v;
  v.slab = (int16_t*)base; base += ((size_t)SF_COUNT * nc * 2 + 15) / 16 * 16;
  v.insub = base; base += ((size_t)nc + 15) / 16 * 16;
  v.head = (StepHeader*)base; base += 128;
  v.snapMu = (double*)base; base += (size_t)nc * 8;
  v.snapCnt = (int32_t*)base; base += ((size_t)nc * 4 + 15) / 16 * 16;
  v.rng = (MTState*)base; base += (sizeof(MTState) + 15) / 16 * 16;
  v.meta = (int32_t*)base;
  return v;
}

#ifndef S4B_RSTORE
#define S4B_RSTORE 2   // residual stores written through (sc1): nothing of them is left dirty for the end-of-kernel write-back (measured -0.15 us per launch)
#endif
__device__ __forceinline__ void store_r(double* p, double x, double y) {
  typedef double d2v __attribute__((ext_vector_type(2)));
  d2v v; v.x = x; v.y = y;
#if S4B_RSTORE == 1
  __builtin_nontemporal_store(v, reinterpret_cast<d2v*>(p));
#elif S4B_RSTORE == 2
  asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(p), "v"(v) : "memory");
#elif S4B_RSTORE == 3
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" :: "v"(p), "v"(v) : "memory");
#else
  *reinterpret_cast<d2v*>(p) = v;
#endif
}

// header of scratch set (lanes < 28), per-tree scalars of tree tn (lanes 40..45), slot count of tree tnn (lane 48), and the
// doubles {cache log prior of tn, sigma} in one gathered load each
static_assert(sizeof(StepHeader) == 112, "gather layout");
__device__ __forceinline__ void step_header_load(StepScalars& g, const BartArrays& a, const StepHeader* head, int tn, int tnn, int lane) {
  const int32_t* tS = a.treeI32; const size_t tT = (size_t)a.T;
  const int32_t* ap = (const int32_t*)head + (lane < 28 ? lane : 0);
  const int f = lane & 7;
  const bool sc = lane >= 40 && lane < 48 && f < TI_COUNT;
  if (sc) ap = tS + (size_t)f * tT + tn;
  if (lane == 48) ap = tS + (size_t)TI_HWM * tT + tnn;
  g.w = (lane < 28 || sc || lane == 48) ? *ap : 0;
  const double* dp = lane == 1 ? a.clogpi + tn : &a.scale->sigma;
  const double d = (lane == 1 || lane == 2) ? *dp : 0.0;
  g.dlo = __double2loint(d); g.dhi = __double2hiint(d);
}
__device__ __forceinline__ void step_header_store(const Proposal& p, int hwm, int nl, int ni, int gr, int gn, double logPi, StepHeader* dst, int lane) {
  int w = 0;
  const int v[28] = {p.type, p.status, p.node, p.var, p.split, p.nbA, p.nbB, p.hwm, p.newLeft, p.newRight, p.pad0, p.pad1,
                     __double2loint(p.priorRatio), __double2hiint(p.priorRatio), __double2loint(p.transRatio), __double2hiint(p.transRatio),
                     __double2loint(p.XLogPi), __double2hiint(p.XLogPi), __double2loint(p.YLogPi), __double2hiint(p.YLogPi),
                     hwm, nl, ni, gr, gn, 1, __double2loint(logPi), __double2hiint(logPi)};
#pragma unroll
  for (int i = 0; i < 28; ++i) w = lane == i ? v[i] : w;
  if (lane < 28) ((int*)dst)[lane] = w;
}

// snapshot of tree t (main arrays -> scratch set t & 1), all threads of the calling workgroup
__device__ __forceinline__ void snapshot_from_main(const BartArrays& a, int t) {
  const StepScratch& c = a.sc[t & 1];
  const int nc = a.nc; const size_t o = (size_t)t * nc;
  for (int i = threadIdx.x; i < nc; i += blockDim.x) {
    c.slab[SF_CVAR * nc + i] = a.var[o + i]; ((uint16_t*)c.slab)[SF_CCUT * nc + i] = a.cut[o + i]; c.slab[SF_CLEFT * nc + i] = a.left[o + i];
    c.slab[SF_CRIGHT * nc + i] = a.right[o + i]; c.slab[SF_CPARENT * nc + i] = a.parent[o + i]; c.slab[SF_CNA * nc + i] = a.cna[o + i];
    c.slab[SF_CDEP * nc + i] = a.cdep[o + i]; c.slab[SF_CLEAF * nc + i] = a.cleaf[o + i]; c.slab[SF_CPRE * nc + i] = a.cpre[o + i];
    c.slab[SF_CPOST * nc + i] = a.cpost[o + i]; c.snapMu[i] = a.mu[o + i]; c.snapCnt[i] = a.cnt[o + i];
  }
  if (threadIdx.x == 0) { c.head->hwm = a.hwm[t]; c.head->nl = a.cnl[t]; c.head->ni = a.cni[t]; c.head->g = a.cg[t]; c.head->gn = a.cgn[t]; c.head->valid = 1; c.head->logPi = a.clogpi[t]; }
}
// structure cache of tree t: snapshot -> main arrays (the wave path keeps a rebuilt cache in the snapshot only)
__device__ __forceinline__ void cache_to_main(const BartArrays& a, int t) {
  const StepScratch& c = a.sc[t & 1];
  const int nc = a.nc; const size_t o = (size_t)t * nc;
  for (int i = threadIdx.x; i < nc; i += blockDim.x) {
    a.cna[o + i] = c.slab[SF_CNA * nc + i]; a.cdep[o + i] = c.slab[SF_CDEP * nc + i]; a.cleaf[o + i] = c.slab[SF_CLEAF * nc + i];
    a.cpre[o + i] = c.slab[SF_CPRE * nc + i]; a.cpost[o + i] = c.slab[SF_CPOST * nc + i];
  }
  if (threadIdx.x == 0) { a.cnl[t] = c.head->nl; a.cni[t] = c.head->ni; a.cg[t] = c.head->g; a.cgn[t] = c.head->gn; a.clogpi[t] = c.head->logPi; a.cvalid[t] = 1; }
}
__device__ __forceinline__ bool step_fits_wave(int need, int nb, int nc) { return need <= 64 && nb <= 64 && need <= nc + 2; }

}  // namespace s4b
#endif
