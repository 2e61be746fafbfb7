// Shared by both translation units of libs4b.so (dev_hip.hip, dev_sweep.hip): the per-node LDS records of the tree passes and the
// wave-register control code (k_control, k_step and k_sweep run the same propose / decide of tree_hd.hpp on it).
// Templates, forceinline functions and types only; control_global_path is the one out-of-line device function (each unit's device
// code object carries its own copy).
#ifndef S4B_DEV_CONTROL_HPP
#define S4B_DEV_CONTROL_HPP

#include <hip/hip_runtime.h>
#include "dev_common.hpp"
#include "dev_wave.hpp"

namespace s4b {

// Per-node tables live in LDS as packed 16-byte records (one ds_read_b128 per observation and half).
struct __attribute__((aligned(16))) NodeS { double mu; int16_t binA, binB; int16_t insub; int16_t pad; };   // stats half
struct __attribute__((aligned(8))) NodeP { int16_t var; uint16_t cut; int16_t left, right; };                // 8 B: routing
static_assert(sizeof(NodeS) == 16 && sizeof(NodeP) == 8, "LDS record sizes are part of the carve layout");
struct __attribute__((aligned(16))) NodeA { double muOld, muNew; };                                           // apply half
static_assert(sizeof(NodeA) == 16, "LDS record sizes are part of the carve layout");

typedef unsigned short us4_t __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------
// The wave-register control code.  The control code is sequential and branchy; run from memory (even LDS) every dependent access costs
// 64+ cycles.  Here every small array of the step (tree structure, proposed tree, bin maps, leaf values) is
// held in ONE VGPR spread across the 64 lanes of the wave — element i lives in lane i — and read with
// v_readlane / written with v_writelane.  All 64 lanes execute the same (wave-uniform) scalar program, so an
// "array access" is a 1-instruction register access.  Trees with more than 64 node slots in use take the
// slower global-memory path (same source, pointer storage).
template <class T>
struct WaveArr {   // up to 64 elements of an integer type of <= 32 bits
  int r;
  __device__ __forceinline__ T get(int i) const { return (T)__builtin_amdgcn_readlane(r, i); }
  __device__ __forceinline__ void set(int i, T v) { r = ((int)(threadIdx.x & 63) == i) ? (int)v : r; }
};
struct WaveArrD {  // up to 64 doubles
  int lo, hi;
  __device__ __forceinline__ double get(int i) const {
    return __hiloint2double(__builtin_amdgcn_readlane(hi, i), __builtin_amdgcn_readlane(lo, i));
  }
  __device__ __forceinline__ void set(int i, double v) {
    const bool me = (int)(threadIdx.x & 63) == i;
    lo = me ? __double2loint(v) : lo;
    hi = me ? __double2hiint(v) : hi;
  }
  __device__ __forceinline__ void load(double v) { lo = __double2loint(v); hi = __double2hiint(v); }
  __device__ __forceinline__ double mine() const { return __hiloint2double(hi, lo); }
};
typedef TreeT<WaveArr<int16_t>, WaveArr<uint16_t>> WaveTree;
typedef StepTablesT<WaveTree, WaveArr<int16_t>, WaveArr<uint8_t>> WaveTables;

// whole-register copy (overload picked over the element-wise template)
__device__ __forceinline__ void tv_copy(const WaveTree& src, WaveTree& dst, int) {
  dst.var.r = src.var.r; dst.cut.r = src.cut.r; dst.left.r = src.left.r; dst.right.r = src.right.r; dst.parent.r = src.parent.r;
  dst.na.r = src.na.r; dst.dep.r = src.dep.r;
}
__device__ __forceinline__ void copy_leaf_values(const WaveArrD& mu, WaveArrD& muOld, int hwm, int) {
  const bool in = (int)(threadIdx.x & 63) < hwm;
  muOld.lo = in ? mu.lo : 0; muOld.hi = in ? mu.hi : 0;
}
// lane-parallel versions of the batched math of decide(): lane b / lane i owns bin b / leaf i
__device__ __forceinline__ void bins_loglik(const WaveArrD& binCnt, const WaveArrD& binSum, const WaveArrD& binWt, int, double sigma2, double prec, WaveArrD& out) {
  const double c = binCnt.mine();
  out.load(c == 0.0 ? 0.0 : leaf_loglik(binWt.mine(), binSum.mine(), sigma2, prec));
}
// value of one leaf from its statistics (weight w, weighted sum s) and the two uniforms of its draw (tree_hd.hpp leaves_draw)
// (in two halves: the standard normal deviate depends on the two uniforms alone — the persistent sweep has it ready before the statistics arrive)
__device__ __forceinline__ double leaf_deviate(double u1, double u2) {
  const double BIG = 134217728.0;
  return r_qnorm(((double)(int)(BIG * u1) + u2) / BIG);
}
// (... and of the posterior only the mean depends on the weighted sum: postPrec = w / sigma2, den = prec + postPrec, sd = 1 / sqrt(den))
__device__ __forceinline__ double leaf_value_parts(double postPrec, double den, double sd, double w, double s, double z) {
  const double mean = postPrec * (s / w) / den;
  return mean + sd * z;
}
__device__ __forceinline__ double leaf_value_z(double w, double s, double z, double sigma2, double prec) {
  const double postPrec = w / sigma2;
  const double den = prec + postPrec;
  const double sd = 1.0 / sqrt(den);
  return leaf_value_parts(postPrec, den, sd, w, s, z);
}
__device__ __forceinline__ double leaf_value(double w, double s, double u1, double u2, double sigma2, double prec) {
  return leaf_value_z(w, s, leaf_deviate(u1, u2), sigma2, prec);
}
__device__ __forceinline__ void leaves_draw(const WaveArrD& lc, const WaveArrD& ls, const WaveArrD& lw, const WaveArrD& u1, const WaveArrD& u2, int nl,
                                            double sigma2, double prec, WaveArrD& out) {
  const double c = lc.mine();
  double v = 0.0;
  if ((int)(threadIdx.x & 63) < nl && c != 0.0) v = leaf_value(lw.mine(), ls.mine(), u1.mine(), u2.mine(), sigma2, prec);
  out.load(v);
}

__device__ __forceinline__ void wave_tree_load(WaveTree& t, const int16_t* var, const uint16_t* cut, const int16_t* left, const int16_t* right,
                                               const int16_t* parent, int count, int nc, int lane) {
  const bool in = lane < count;
  t.var.r = in ? (int)var[lane] : (int)NODE_FREE; t.cut.r = in ? (int)cut[lane] : 0; t.left.r = in ? (int)left[lane] : -1;
  t.right.r = in ? (int)right[lane] : -1; t.parent.r = in ? (int)parent[lane] : -1; t.na.r = 0; t.dep.r = 0; t.nc = nc < 64 ? nc : 64;
}
__device__ __forceinline__ void wave_tree_store(const WaveTree& t, int16_t* var, uint16_t* cut, int16_t* left, int16_t* right, int16_t* parent,
                                                int count, int lane) {
  if (lane < count) { var[lane] = (int16_t)t.var.r; cut[lane] = (uint16_t)t.cut.r; left[lane] = (int16_t)t.left.r; right[lane] = (int16_t)t.right.r;
                      parent[lane] = (int16_t)t.parent.r; }
}

// slow path for trees with more than 64 node slots in use: the sequential code straight on the global arrays
__device__ __attribute__((noinline)) void control_global_path(BartArrays a, int t, int next, double* scratch) {
  a.model.scratch = scratch;
  if (t >= 0) control_step(a, t, next); else propose_step(a, next);
}

typedef TreeCacheT<WaveArr<int16_t>> WaveCache;

// Generator as the control wave sees it: the state array stays in LDS, the position and the 64-word window
// around it live in registers (lane l = mt[wbase + l]), so a draw is a v_readlane plus the tempering.
struct WaveRng {
  MTState* st; int mti; int wbase; uint32_t win; int count; int regen;   // count: draws since open() / since last zeroed; regen: the block was regenerated
  __device__ __forceinline__ void open(MTState* s) { st = s; mti = S4B_UNI((int)s->mti); wbase = -64; win = 0u; count = 0; regen = 0; }
  __device__ __forceinline__ void close() { st->mti = mti; }
};
__device__ __forceinline__ uint32_t mt_next(WaveRng* r) {
  int k = r->mti;
  if (k >= 624) { mt_regenerate_wave(r->st); k = 0; r->wbase = -64; r->regen = 1; }
  const int wb = k & ~63;
  if (wb != r->wbase) {
    const int idx = wb + (int)(threadIdx.x & 63);
    r->win = idx < 624 ? r->st->mt[idx] : 0u;
    r->wbase = wb;
  }
  uint32_t y = (uint32_t)__builtin_amdgcn_readlane((int)r->win, k & 63);
  r->mti = k + 1; ++r->count;
  y ^= (y >> 11);
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= (y >> 18);
  return y;
}

// lane-parallel leaf statistics + draws of decide(): lane i owns leaf i of the cached DFS list.  The uniforms are the generator's
// next words in leaf order (two per leaf that holds observations): lane i reads the pair at its rank among those leaves.
__device__ __forceinline__ int wave_gather(int idx, int v) { return __builtin_amdgcn_ds_bpermute(idx << 2, v); }
__device__ __forceinline__ double wave_gather(int idx, const WaveArrD& a) { return __hiloint2double(wave_gather(idx, a.hi), wave_gather(idx, a.lo)); }
__device__ __forceinline__ double mt_word_to_unif(uint32_t y) {
  y ^= (y >> 11);
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= (y >> 18);
  const double half_ulp = 0.5 * 2.328306437080797e-10;
  const double v = (double)y * 2.3283064365386963e-10;
  return v <= 0.0 ? half_ulp : (1.0 - v <= 0.0 ? 1.0 - half_ulp : v);
}
__device__ __forceinline__ void leaf_stats_draws(const WaveTables& tb, const WaveCache& ca, const WaveArrD& binCnt, const WaveArrD& binSum, const WaveArrD& binWt,
                                                 bool acc, bool deathAcc, int nd, double cDeath, double sDeath, double wDeath, DecideWork<WaveArrD>& wk, WaveRng* rng) {
  const int lane = (int)(threadIdx.x & 63);
  const int nl = ca.nl;
  const bool in = lane < nl;
  const int n = in ? ca.leaf.r : 0;
  const int bB = (int)(int16_t)wave_gather(n, tb.binB.r), bA = (int)(int16_t)wave_gather(n, tb.binA.r);
  const int b = ((acc && !deathAcc && bB >= 0) ? bB : bA) & 63;
  double lc = wave_gather(b, binCnt), ls = wave_gather(b, binSum), lw = wave_gather(b, binWt);
  const bool dn = deathAcc && n == nd;
  lc = dn ? cDeath : lc; ls = dn ? sDeath : ls; lw = dn ? wDeath : lw;
  const bool ne = in && lc != 0.0;
  const unsigned long long mask = __ballot(ne);
  const int cnt = __popcll(mask);
  if (rng->mti + 2 * cnt > 624) {   // the block of words runs out among these draws (about one step in a hundred): one draw at a time
    leaf_stats_draws<WaveTables, WaveCache, WaveArrD, WaveArrD, WaveRng>(tb, ca, binCnt, binSum, binWt, acc, deathAcc, nd, cDeath, sDeath, wDeath, wk, rng);
    return;
  }
  const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
  const int k = ne ? rng->mti + 2 * rank : 0;
  const uint32_t y1 = rng->st->mt[k], y2 = rng->st->mt[k + 1];
  if (in) { wk.lc.load(lc); wk.ls.load(ls); wk.lw.load(lw); }
  if (ne) { wk.u1.load(mt_word_to_unif(y1)); wk.u2.load(mt_word_to_unif(y2)); }
  rng->mti += 2 * cnt; rng->count += 2 * cnt; rng->wbase = -64;
}

// Model view of the control wave: the prior tables sit in registers (lane d / lane k), LDS only beyond 64 / 128
// (SPL: cgm(split.probs) — the weighted predictor choice — on the wave-register path: only the persistent sweep's kernels k_sweep_sp /
// k_sweep_few_sp are compiled with it; everywhere else the wave-register code is compiled without and such samplers take the
// pointer-storage control code)
template <bool SPL>
struct WaveModelT : ModelView {
  WaveArrD pg, lpg, l1pg, li0, li1; int nc0, nc1;
};
// (with the weights: spTab, on chip — [0, 128) the running sum of the weights through predictor v over the predictors that have cuts, in predictor order;
// [128, 256) log(weight of predictor v); [256] the sum over all of them, [257] its logarithm: what the sums below come to at a node where every predictor
// is still available, which is nearly every node — k_sweep_sp's prologue fills it)
template <>
struct WaveModelT<true> : ModelView {
  WaveArrD pg, lpg, l1pg, li0, li1; int nc0, nc1; const double* spTab;
};
constexpr int SP_TAB = 258;
typedef WaveModelT<false> WaveModel;
template <bool SPL> __device__ __forceinline__ double mv_pg_depth(const WaveModelT<SPL>& m, int d) { return d < 64 ? m.pg.get(d) : S4B_UNI(m.pgDepth[d]); }
template <bool SPL> __device__ __forceinline__ double mv_log_pg(const WaveModelT<SPL>& m, int d) { return d < 64 ? m.lpg.get(d) : S4B_UNI(m.logPg[d]); }
template <bool SPL> __device__ __forceinline__ double mv_log1m_pg(const WaveModelT<SPL>& m, int d) { return d < 64 ? m.l1pg.get(d) : S4B_UNI(m.log1mPg[d]); }
template <bool SPL> __device__ __forceinline__ double mv_log_int(const WaveModelT<SPL>& m, int k) {
  return k < 64 ? m.li0.get(k) : (k < 128 ? m.li1.get(k - 64) : S4B_UNI(m.logInt[k]));
}
template <bool SPL> __device__ __forceinline__ const double* mv_split_probs(const WaveModelT<SPL>& m) { return SPL ? m.splitProbs : nullptr; }
template <bool SPL> __device__ __forceinline__ int mv_num_cuts(const WaveModelT<SPL>& m, int v) {
  return v < 64 ? __builtin_amdgcn_readlane(m.nc0, v) : (v < 128 ? __builtin_amdgcn_readlane(m.nc1, v - 64) : S4B_UNI(m.numCuts[v]));
}

// cgm(split.probs) on the wave-register path.  Which predictors still have a free cut at node n: lane l answers for predictor 64 chunk + l — the walk up
// the ancestors is uniform (register reads), every lane narrows the interval of ITS predictor (tv_interval for 64 predictors at once).  The sums over the
// available predictors are then formed in increasing predictor order, one add per available predictor, exactly as the sequential tv_avail_prob_sum and
// tv_draw_var of tree_hd.hpp form them: the same doubles, the same draw.  (The sequential versions walk the ancestors once per predictor through register
// reads: 59 us per tree update at P = 49 against 8 without the weights; these: see DESIGN.md 8.)
__device__ __forceinline__ unsigned long long wave_avail_mask(const WaveTree& t, const WaveModelT<true>& m, int n, int chunk) {
  const int v = chunk * 64 + (int)(threadIdx.x & 63);
  const int ncv = chunk == 0 ? m.nc0 : (chunk == 1 ? m.nc1 : (v < m.P ? m.numCuts[v] : 0));
  int lo = 0, hi = ncv - 1;
  int child = n;
  for (int a = t.parent.get(n); a >= 0; child = a, a = t.parent.get(a)) {
    const int av = t.var.get(a), s = (int)t.cut.get(a);
    const bool isLeft = child == t.left.get(a);
    const bool hit = av == v;
    hi = (hit && isLeft && s - 1 < hi) ? s - 1 : hi;
    lo = (hit && !isLeft && s + 1 > lo) ? s + 1 : lo;
  }
  return __ballot(v < m.P && ncv > 0 && lo <= hi);
}
__device__ __forceinline__ double wave_lane_double(double x, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}
__device__ __forceinline__ double tv_avail_prob_sum(const WaveTree& t, const WaveModelT<true>& m, int n, const double* sp) {
  if ((int)t.na.get(n) == m.Pvalid) return S4B_UNI(m.spTab[256]);      // nothing exhausted on the way down to n: the sum over all, formed once
  double tot = 0.0;
  for (int c = 0; c * 64 < m.P; ++c) {
    unsigned long long mask = wave_avail_mask(t, m, n, c);
    const int v = c * 64 + (int)(threadIdx.x & 63);
    const double mine = v < m.P ? sp[v] : 0.0;
    while (mask) {
      const int b = __builtin_amdgcn_readfirstlane(__ffsll((long long)mask) - 1);
      mask &= mask - 1ull;
      tot += wave_lane_double(mine, b);
    }
  }
  return tot;
}
__device__ __forceinline__ double tv_log_var_prob(const WaveTree& t, const WaveModelT<true>& m, int n, int v, int na) {
  const double* sp = m.splitProbs;
  if (!sp) return -mv_log_int(m, na);
  const double lv = v < 128 ? S4B_UNI(m.spTab[128 + v]) : log(S4B_UNI(sp[v]));
  if (na == m.Pvalid) return lv - S4B_UNI(m.spTab[257]);
  return lv - log(tv_avail_prob_sum(t, m, n, sp));
}
// (k_sweep_sp's prologue, one wave: the table of the weights)
__device__ __forceinline__ void wave_fill_sp_tab(const BartArrays& a, double* spTab, int lane) {
  const double* sp = a.model.splitProbs;
  double run = 0.0;
  for (int c = 0; c * 64 < a.P; ++c) {
    const int v = c * 64 + lane;
    const bool ok = v < a.P && a.numCuts[v] > 0;
    const double mine = v < a.P ? sp[v] : 1.0;
    unsigned long long mask = __ballot(ok);
    double pre = run;
    while (mask) {
      const int b = __builtin_amdgcn_readfirstlane(__ffsll((long long)mask) - 1);
      mask &= mask - 1ull;
      run += wave_lane_double(mine, b);
      pre = lane >= b ? run : pre;
    }
    if (c < 2) { spTab[v] = pre; spTab[128 + v] = log(mine); }
  }
  if (lane == 0) { spTab[256] = run; spTab[257] = log(run); }
}
template <class RNG>
__device__ __forceinline__ int tv_draw_var(const WaveTree& t, const WaveModelT<true>& m, int n, RNG* rng) {
  const double* sp = m.splitProbs;
  if (!sp) { const int good = tv_num_avail(t, m, n); const int idx = r_unif_int(rng, 0, good); return tv_nth_avail_var(t, m, n, idx); }
  const double u = r_unif(rng) * tv_avail_prob_sum(t, m, n, sp);
  if ((int)t.na.get(n) == m.Pvalid && m.P <= 128) {
    // every predictor with cuts is available: the running sums are the table's — the first one beyond u, else the last predictor with cuts
    const int l = (int)(threadIdx.x & 63);
    const bool ok0 = l < m.P && m.nc0 > 0, ok1 = 64 + l < m.P && m.nc1 > 0;
    const unsigned long long v0 = __ballot(ok0), v1 = __ballot(ok1);
    const unsigned long long h0 = __ballot(ok0 && m.spTab[l] > u), h1 = __ballot(ok1 && m.spTab[64 + l] > u);
    if (h0) return __builtin_amdgcn_readfirstlane(__ffsll((long long)h0) - 1);
    if (h1) return __builtin_amdgcn_readfirstlane(64 + __ffsll((long long)h1) - 1);
    if (v1) return __builtin_amdgcn_readfirstlane(127 - __clzll((long long)v1));
    return v0 ? __builtin_amdgcn_readfirstlane(63 - __clzll((long long)v0)) : -1;
  }
  double run = 0.0; int last = -1;
  for (int c = 0; c * 64 < m.P; ++c) {
    unsigned long long mask = wave_avail_mask(t, m, n, c);
    const int v = c * 64 + (int)(threadIdx.x & 63);
    const double mine = v < m.P ? sp[v] : 0.0;
    while (mask) {
      const int b = __builtin_amdgcn_readfirstlane(__ffsll((long long)mask) - 1);
      mask &= mask - 1ull;
      run += wave_lane_double(mine, b); last = c * 64 + b;
      if (__builtin_amdgcn_readfirstlane((int)(run > u))) return last;
    }
  }
  return last;
}

// Workgroup of 8 waves with fixed roles, tied together by two LDS hand-shakes (no workgroup barrier after start-up):
//   wave 0        decide(t): waits for the bin totals, accept/reject, leaf draws, writes tree t, names the winner
//   waves 1, 2    candidates (waves are dealt round-robin to the 4 SIMDs: the three long-running roles sit on three SIMDs): draw the proposal of tree `next` from the generator position decide(t) will leave behind —
//                 that position is known up to one bit before the statistics arrive: decide consumes one uniform for the
//                 accept test plus two per leaf of the tree it ends with, i.e. d + 2 nl (reject) or d + 2 nl' (accept).
//                 Each candidate advances a private copy of the generator by its hypothesis and runs propose() while
//                 wave 0 is still waiting / deciding; the one whose hypothesis matches the draws actually consumed
//                 publishes its tables and generator state.  A leaf without observations (no draw) breaks both
//                 hypotheses: then wave 0 proposes itself, as it does at the start of a sweep.
//   waves 3-7     reducers: per-workgroup partials -> bin totals (fixed order)
constexpr int CBLOCK = 512;
constexpr int C_NRED = 5;
struct ControlShared {
  MTState rng[3];                        // slot 0: wave 0, slots 1, 2: candidates
  double scratch[3][S4B_MAX_DEPTH];
  double red[3][C_NRED][64];             // [sum | count | weight][reducer][bin]
  Proposal prT, prN[3];
  int arrived, verdict;
  long long tPost, tStart0;
};
__device__ __forceinline__ void rng_advance(WaveRng* r, int k) {
  int total = r->mti + k;
  while (total > 624) { mt_regenerate_wave(r->st); total -= 624; r->regen = 1; }
  r->mti = total; r->wbase = -64;
}

// the step's scalars in one gathered load: lane l < 20 holds dword l of the pending Proposal of tree tt, lanes 32.. / 40..
// the int32 per-tree scalars (row TI_x) of trees tt / tn; a second 8-byte gather brings the two log priors and sigma
static_assert(sizeof(Proposal) == 80, "gather layout");
struct StepScalars {
  int w; int dlo, dhi;
  __device__ __forceinline__ int i32(int l) const { return __builtin_amdgcn_readlane(w, l); }
  __device__ __forceinline__ double f64w(int l) const { return __hiloint2double(__builtin_amdgcn_readlane(w, l + 1), __builtin_amdgcn_readlane(w, l)); }
  __device__ __forceinline__ double f64(int l) const { return __hiloint2double(__builtin_amdgcn_readlane(dhi, l), __builtin_amdgcn_readlane(dlo, l)); }
  __device__ __forceinline__ void proposal(Proposal& p) const {
    p.type = i32(0); p.status = i32(1); p.node = i32(2); p.var = i32(3); p.split = i32(4); p.nbA = i32(5); p.nbB = i32(6); p.hwm = i32(7);
    p.newLeft = i32(8); p.newRight = i32(9); p.pad0 = i32(10); p.pad1 = i32(11);
    p.priorRatio = f64w(12); p.transRatio = f64w(14); p.XLogPi = f64w(16); p.YLogPi = f64w(18);
  }
};
__device__ __forceinline__ void step_scalars_load(StepScalars& g, const BartArrays& a, const Proposal* prop, int tt, int tn, int lane, bool withDoubles) {
  const int32_t* tS = a.treeI32; const size_t tT = (size_t)a.T;
  const int32_t* ap = (const int32_t*)prop + (lane < 20 ? lane : 0);
  const int f = lane & 7;
  if (lane >= 32 && lane < 48 && f < TI_COUNT) ap = tS + (size_t)f * tT + (lane < 40 ? tt : tn);
  g.w = (lane < 20 || (lane >= 32 && lane < 48 && f < TI_COUNT)) ? *ap : 0;
  g.dlo = 0; g.dhi = 0;
  if (withDoubles) {
    const double* dp = lane == 0 ? a.clogpi + tt : (lane == 1 ? a.clogpi + tn : &a.scale->sigma);
    const double d = lane < 3 ? *dp : 0.0;
    g.dlo = __double2loint(d); g.dhi = __double2hiint(d);
  }
}
// proposal record -> global, one dword per lane
__device__ __forceinline__ void proposal_store(const Proposal& p, Proposal* dst, int lane) {
  int w = 0;
  const int v[20] = {p.type, p.status, p.node, p.var, p.split, p.nbA, p.nbB, p.hwm, p.newLeft, p.newRight, p.pad0, p.pad1,
                     __double2loint(p.priorRatio), __double2hiint(p.priorRatio), __double2loint(p.transRatio), __double2hiint(p.transRatio),
                     __double2loint(p.XLogPi), __double2hiint(p.XLogPi), __double2loint(p.YLogPi), __double2hiint(p.YLogPi)};
#pragma unroll
  for (int i = 0; i < 20; ++i) w = lane == i ? v[i] : w;
  if (lane < 20) ((int*)dst)[lane] = w;
}

}  // namespace s4b
#endif
