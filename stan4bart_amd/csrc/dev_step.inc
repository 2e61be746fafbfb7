// k_step: the fused tree update — ONE launch per tree of the sweep (included once, by dev_hip.hip, after dev_step_shared.hpp).
//
// A tree update is the dependent chain  statistics(t-1) -> decide(t-1) -> leaf values -> residual -> statistics(t).  With two
// kernels per tree (k_tree + k_control) the chain pays two kernel boundaries, a one-workgroup launch and two cold hops for the
// tables per tree: at n = 1e6 that is 22 us for 2.75 us worth of HBM traffic.  Launch t of the fused path has gridDim.x - 1 PASS
// workgroups, which share the observations, and one CONTROL workgroup (the last), which owns none.  In a pass workgroup:
//     waves 3-7   combine the per-workgroup partials of statistics(t-1) in a fixed order, then request the workgroup's
//                 observations (residual, both leaf planes: nothing of that depends on the pending decision);
//     wave 0      decide(t-1) from the bin totals (accept / reject, leaf draws);
//     waves 1-2   fetch one IMAGE each of the proposal of tree t — it was drawn during launch t-1, once per number of draws
//                 decide(t-1) can consume — stage its tables, wait for the verdict (which image matches the draws consumed);
//     all         one barrier; then the O(N) pass: finish tree t-1 (residual update, relabelling) and gather the statistics of
//                 tree t under the surviving proposal, from tables that never left the workgroup (LDS).
// The control workgroup decides like the others, writes the results back (tree t-1 to the main arrays, the surviving image into
// scratch set t & 1, its generator state into the stream slot of launch t+1) and draws the two images of tree t+1 while the others
// run the pass — a first attempt, assuming image 0 of tree t survives, already runs beside decide().  No proposal is drawn on the
// critical path; wave 0 proposes itself only at the start of a sweep, after a step on the global-memory path, or when no image
// matches.  The control code is deterministic, so every workgroup computes the same decision from the same inputs.
// What a launch reads is never written by the same launch: the decided tree goes to the main arrays while every workgroup
// reads its pre-decision snapshot from the scratch set; partials, generator slots and images alternate by launch parity.
// The memory latency of the pass hides behind the control code, one kernel boundary per tree is gone, and so are the hops
// control kernel -> global -> tree kernel -> LDS.
//
// Trees that do not fit the wave-register control path (> 64 node slots in use): the launch that discovers it (it knows the
// sizes one step ahead) lets its LAST finishing workgroup (device-scope ticket) run the sequential global-memory control code
// for the next step and raises preDone; the next launch then only stages tables from global memory, like k_tree does.
namespace s4b {
constexpr int F_PT = FBLOCK;         // pass threads per workgroup: thread tau owns quads b * 512 + tau + j * ((grid - 1) * 512)
constexpr int F_PF = 2;              // quads per thread that are requested before the control code runs
constexpr int F_CTL = 3 * 64;        // threads of the control waves: their first quads are requested by the loader waves and
                                     // handed over through LDS (the control code needs the registers)
#ifndef S4B_F_SECOND
#define S4B_F_SECOND 0
#endif
constexpr bool F_SECOND = S4B_F_SECOND != 0;   // second routing level prefetched with the first
constexpr int F_GRID_MAX = 640;      // partials per bin the reducers combine (two per reducer lane)

// paGo: the proposal of tree tn is settled (F.root .. F.sset, F.pa* = its type / status / leaf count, generator state in S.rng[F.sset])
struct StepShared { int prevAcc, prevRoot, hp, root, nb, hwmS, needBig, last, sset, paGo, paType, paStatus, paNbA; MTState rngB[2]; };

__host__ __device__ static inline size_t step_lds_bytes(int nc, bool weighted) {
  return (size_t)nc * (3 * (16 + 8) + 16 + 8) + ((size_t)nc + 15) / 16 * 16 + 8 * 16 * 8 + 8 * 16 * 8 + 8 * 16 * 4 +
         (size_t)F_PF * F_CTL * (weighted ? 80 : 48);
}
// S / SP: the statistics-half tables the pass uses; every proposing wave fills its own set S3[slot] / SP3[slot] as soon as its
// proposal is drawn (before it knows whether its speculation holds), the surviving one is selected after the barrier
struct StepLds { NodeS* S; NodeP* SP; NodeS* S3; NodeP* SP3; NodeA* A;   // set k: S3 + k * nc, SP3 + k * nc
                 NodeP* AP; uint8_t* Ain; double* redS; double* redW; int* redN;
                 double2* hR01; double2* hR23; us4_t* hLf; us4_t* hPl; double2* hW01; double2* hW23; };
__device__ __forceinline__ StepLds carve_step(unsigned char* base, int nc) {
  StepLds L;
  L.S3 = (NodeS*)base; base += (size_t)3 * nc * 16;
  L.A = (NodeA*)base; base += (size_t)nc * 16;
  L.SP3 = (NodeP*)base; base += (size_t)3 * nc * 8;
  L.AP = (NodeP*)base; base += (size_t)nc * 8;
  L.S = L.S3; L.SP = L.SP3;
  L.Ain = (uint8_t*)base; base += ((size_t)nc + 15) / 16 * 16;
  L.redS = (double*)base; base += 8 * 16 * 8;
  L.redW = (double*)base; base += 8 * 16 * 8;
  L.redN = (int*)base; base += 8 * 16 * 4;
  // hand-over slots [j][control thread]: structure of arrays, 16-byte aligned
  L.hR01 = (double2*)base; base += (size_t)F_PF * F_CTL * 16;
  L.hR23 = (double2*)base; base += (size_t)F_PF * F_CTL * 16;
  L.hLf = (us4_t*)base; base += (size_t)F_PF * F_CTL * 8;
  L.hPl = (us4_t*)base; base += (size_t)F_PF * F_CTL * 8;
  L.hW01 = (double2*)base; base += (size_t)F_PF * F_CTL * 16;   // (only carved for, and touched by, the weighted kernel)
  L.hW23 = (double2*)base;
  return L;
}

#ifdef S4B_LIGHT_TIMING
// (light measurement build, `make light`: one time stamp per wave right before the main barrier and one at the end of the pass, taken
// in one pass workgroup; nothing else is perturbed)  [0..7] arrival of wave w, [8] end of the pass, [9] launches
__device__ unsigned long long g_arr[16];
#define S4B_ARRIVE() do { tArr = wall_clock64(); } while (0)
#else
#define S4B_ARRIVE()
#endif
#ifdef S4B_CONTROL_TIMING
// phase timers of k_step (100 MHz wall clock), summed over workgroups / launches: [0] launches x workgroups, [1] reducers done,
// [2] decider loads, [3] decider got the totals, [4] decide done, [5] decider stores done, [6] winner propose done, [7] winner
// stores done, [8] barrier passed, [9] pass done; [10] min / [11] max workgroup start, [12] max end (absolute, last launch)
__device__ unsigned long long g_step[32];
__device__ unsigned long long g_wgS[F_GRID_MAX], g_wgE[F_GRID_MAX];   // per workgroup: sums of absolute start / end times
#define S4B_STEP_T(i) do { if (doDecide && doPropose && (int)blockIdx.x == S4B_TIMED_WG) atomicAdd(&g_step[i], (unsigned long long)(wall_clock64() - tq0)); } while (0)
#define S4B_CTL_T(i) do { if (doDecide && doPropose && ctl) atomicAdd(&g_step[i], (unsigned long long)(wall_clock64() - tq0)); } while (0)
#define S4B_PASS_T(i) do { if (APPLY && STATS && USEPRE && (int)blockIdx.x == S4B_TIMED_WG && threadIdx.x == 3 * 64) { __builtin_amdgcn_sched_barrier(0); atomicAdd(&g_step[i], (unsigned long long)wall_clock64()); __builtin_amdgcn_sched_barrier(0); } } while (0)
#ifndef S4B_TIMED_WG
#define S4B_TIMED_WG 0
#endif
#else
#define S4B_STEP_T(i)
#define S4B_CTL_T(i)
#define S4B_PASS_T(i)
#endif

template <bool WEIGHTED>
struct StepPre { double2 r01[F_PF], r23[F_PF]; us4_t lf4[F_PF], pl4[F_PF]; double2 w01[WEIGHTED ? F_PF : 1], w23[WEIGHTED ? F_PF : 1]; };

// the O(N) pass of one launch for bins [base, base + NB): apply half for tree tA (APPLY), statistics half for tree tS (STATS).
// Pass thread `q0, q0 + stride, ...` are its quads (q0 >= nQuads: none — the control waves); with USEPRE the first F_PF of
// them were requested before the control code ran and sit in P.
template <int NB, bool APPLY, bool STATS, bool WEIGHTED, bool USEPRE>
__device__ __forceinline__ void step_pass(const BartArrays& a, int tS, int tA, const StepLds& L, int root, int prevRoot, int prevAcc, int base,
                                          int nbTotal, const StepPre<WEIGHTED>& P, int64_t q0, int64_t stride, double* part) {
  // per-thread sums and counts (counts as doubles: exact, and one add with the factor the sum's fused multiply-add uses anyway)
  double accS[NB]; double accC[NB]; double accW[WEIGHTED ? NB : 1];
#pragma unroll
  for (int k = 0; k < NB; ++k) { accS[k] = 0.0; accC[k] = 0.0; if (WEIGHTED) accW[k] = 0.0; }
  const double* __restrict__ W = a.wts;
  const int64_t nQuads = (a.n + 3) >> 2;
  const uint16_t* __restrict__ leafPlane = a.leaf + (size_t)tS * a.npad;
  uint16_t* __restrict__ prevPlane = a.leaf + (size_t)tA * a.npad;
  double* __restrict__ R = a.R;
  const int rootVarS = STATS ? (int)L.SP[root].var : -1;
  const int rootCutS = STATS ? (int)L.SP[root].cut : 0, rootLS = STATS ? (int)L.SP[root].left : 0, rootRS = STATS ? (int)L.SP[root].right : 0;
  const int rootVarA = (APPLY && prevAcc) ? (int)L.AP[prevRoot].var : -1;
  const int rootCutA = APPLY ? (int)L.AP[prevRoot].cut : 0, rootLA = APPLY ? (int)L.AP[prevRoot].left : 0, rootRA = APPLY ? (int)L.AP[prevRoot].right : 0;
  const uint16_t* __restrict__ colS = a.xbin + (size_t)(rootVarS >= 0 ? rootVarS : 0) * a.npad;
  const uint16_t* __restrict__ colA = a.xbin + (size_t)(rootVarA >= 0 ? rootVarA : 0) * a.npad;

  // arithmetic of one quad once both routings are known: nlA[e] = leaf of observation e in the decided tree t-1, ndS[e] = leaf the
  // pending proposal of tree t sends it to (-1: it is not under the proposal's node)
  auto accumulate = [&](int64_t qd, double2 r01, double2 r23, us4_t lf4, us4_t pl4, const unsigned (&nlA)[4], const int (&ndS)[4], double2 w01, double2 w23) {
    const int64_t i0 = qd << 2;
    double rr[4] = {r01.x, r01.y, r23.x, r23.y};
    const double ww[4] = {w01.x, w01.y, w23.x, w23.y};
    const unsigned lf[4] = {lf4.x, lf4.y, lf4.z, lf4.w};
    const unsigned pl[4] = {pl4.x, pl4.y, pl4.z, pl4.w};
    const int valid = (a.n - i0) >= 4 ? 4 : (int)(a.n - i0);
    if (APPLY) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned l = e < valid ? pl[e] : 0u;
        const unsigned nl = e < valid ? nlA[e] : 0u;
        rr[e] = (rr[e] + L.A[l].muOld) - L.A[nl].muNew;
      }
      store_r(R + i0, rr[0], rr[1]); store_r(R + i0 + 2, rr[2], rr[3]);
      if (prevAcc) { us4_t o4; o4.x = (unsigned short)nlA[0]; o4.y = (unsigned short)nlA[1]; o4.z = (unsigned short)nlA[2]; o4.w = (unsigned short)nlA[3];
                     __builtin_nontemporal_store(o4, reinterpret_cast<us4_t*>(prevPlane + i0)); }
    }
    if (STATS) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool ok = e < valid;
        const NodeS ns = L.S[ok ? lf[e] : 0u];
        const double r0 = WEIGHTED ? (rr[e] + ns.mu) * ww[e] : rr[e] + ns.mu;
        const double r = ok ? r0 : 0.0;
        const int ba = ok ? (int)ns.binA - base : -1;
        const int bb = (ok && ndS[e] >= 0) ? (int)L.S[ndS[e]].binB - base : -1 - base;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          // acc += match ? r : 0 as ONE fused multiply-add with the match as a 0.0 / 1.0 factor (exact: the product is r or 0)
          const bool m = (ba == k) | (bb == k);
          const double md = __hiloint2double(m ? 0x3ff00000 : 0, 0);
          accS[k] = fma(md, r, accS[k]);
          accC[k] += md;
          if (WEIGHTED) accW[k] = fma(md, ww[e], accW[k]);
        }
      }
    }
  };
  // routing of one quad with dependent loads below the first level (quads beyond the prefetched ones)
  auto process = [&](int64_t qd, double2 r01, double2 r23, us4_t lf4, us4_t pl4, us4_t xs4, us4_t xa4, double2 w01, double2 w23) {
    const int64_t i0 = qd << 2;
    const unsigned lf[4] = {lf4.x, lf4.y, lf4.z, lf4.w};
    const unsigned pl[4] = {pl4.x, pl4.y, pl4.z, pl4.w};
    const unsigned xs[4] = {xs4.x, xs4.y, xs4.z, xs4.w};
    const unsigned xa[4] = {xa4.x, xa4.y, xa4.z, xa4.w};
    const int valid = (a.n - i0) >= 4 ? 4 : (int)(a.n - i0);
    unsigned nlA[4]; int ndS[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      nlA[e] = pl[e]; ndS[e] = -1;
      if (APPLY && prevAcc && e < valid && L.Ain[pl[e]]) {
        int nd = prevRoot;
        if (rootVarA >= 0) nd = (xa[e] <= (unsigned)rootCutA) ? rootLA : rootRA;
        NodeP p = L.AP[nd];
        while (p.var >= 0) {
          const unsigned x = a.xbin[(size_t)p.var * a.npad + (size_t)(i0 + e)];
          nd = (x <= (unsigned)p.cut) ? p.left : p.right;
          p = L.AP[nd];
        }
        nlA[e] = (unsigned)nd;
      }
      if (STATS && e < valid && L.S[lf[e]].insub) {
        int nd = root;
        if (rootVarS >= 0) nd = (xs[e] <= (unsigned)rootCutS) ? rootLS : rootRS;
        NodeP p = L.SP[nd];
        while (p.var >= 0) {
          const unsigned x = a.xbin[(size_t)p.var * a.npad + (size_t)(i0 + e)];
          nd = (x <= (unsigned)p.cut) ? p.left : p.right;
          p = L.SP[nd];
        }
        ndS[e] = nd;
      }
    }
    accumulate(qd, r01, r23, lf4, pl4, nlA, ndS, w01, w23);
  };

  const double2 one2 = make_double2(1.0, 1.0);
  us4_t zero4; zero4.x = 0; zero4.y = 0; zero4.z = 0; zero4.w = 0;
  int64_t qStart = q0;
  S4B_PASS_T(10);
  if (USEPRE) {
    // Routing of all prefetched observations level by level: the loads of one level (every observation of the thread that is
    // still inside the moved subtree, both halves) are in flight together, so a subtree of depth d costs d memory round trips
    // per thread, not d per observation.  First level: the root rules are known up front.  Every table record is read once
    // (16-byte LDS reads) and kept in registers for the arithmetic.
    // Second level: the rules of the root's children are known too; their predictor columns travel in the same round trip
    // (only where a child is an internal node), so that only subtrees deeper than two levels need dependent loads.
    const int varSL = (F_SECOND && STATS && rootVarS >= 0) ? (int)L.SP[rootLS].var : -1, varSR = (F_SECOND && STATS && rootVarS >= 0) ? (int)L.SP[rootRS].var : -1;
    const int varAL = (F_SECOND && APPLY && rootVarA >= 0) ? (int)L.AP[rootLA].var : -1, varAR = (F_SECOND && APPLY && rootVarA >= 0) ? (int)L.AP[rootRA].var : -1;
    us4_t xs[F_PF], xa[F_PF], xs2[2][F_PF], xa2[2][F_PF];
#pragma unroll
    for (int j = 0; j < F_PF; ++j) {
      const int64_t qd = q0 + (int64_t)j * stride;
      xs[j] = zero4; xa[j] = zero4; xs2[0][j] = zero4; xs2[1][j] = zero4; xa2[0][j] = zero4; xa2[1][j] = zero4;
      if (qd < nQuads) {
        if (STATS && rootVarS >= 0) xs[j] = *reinterpret_cast<const us4_t*>(colS + (qd << 2));
        if (APPLY && rootVarA >= 0) xa[j] = *reinterpret_cast<const us4_t*>(colA + (qd << 2));
        if (STATS && varSL >= 0) xs2[0][j] = *reinterpret_cast<const us4_t*>(a.xbin + (size_t)varSL * a.npad + (qd << 2));
        if (STATS && varSR >= 0) xs2[1][j] = *reinterpret_cast<const us4_t*>(a.xbin + (size_t)varSR * a.npad + (qd << 2));
        if (APPLY && varAL >= 0) xa2[0][j] = *reinterpret_cast<const us4_t*>(a.xbin + (size_t)varAL * a.npad + (qd << 2));
        if (APPLY && varAR >= 0) xa2[1][j] = *reinterpret_cast<const us4_t*>(a.xbin + (size_t)varAR * a.npad + (qd << 2));
      }
    }
#ifdef S4B_CONTROL_TIMING
    if (APPLY && STATS && (int)blockIdx.x == S4B_TIMED_WG && threadIdx.x == 3 * 64) { __builtin_amdgcn_s_waitcnt(0); }
    S4B_PASS_T(11);
#endif
    typedef double d2_t __attribute__((ext_vector_type(2)));
    typedef int i4_t __attribute__((ext_vector_type(4)));
    double muOldV[F_PF][4], muNewV[F_PF][4], muS[F_PF][4]; int binAV[F_PF][4], binBV[F_PF][4];
    unsigned nlA[F_PF][4]; int ndS[F_PF][4];
    // The first level sends an observation to one of TWO nodes per side (the children of the move's node): what the pass needs of
    // them — is it a leaf, its new value, its bin — is wave-uniform and fetched once, not once per observation.
    const int cLA = rootVarA >= 0 ? rootLA : prevRoot, cRA = rootVarA >= 0 ? rootRA : prevRoot;
    const int cLS = rootVarS >= 0 ? rootLS : root, cRS = rootVarS >= 0 ? rootRS : root;
    const bool leafLA = APPLY ? (int)L.AP[cLA].var < 0 : true, leafRA = APPLY ? (int)L.AP[cRA].var < 0 : true;
    const bool leafLS = STATS ? (int)L.SP[cLS].var < 0 : true, leafRS = STATS ? (int)L.SP[cRS].var < 0 : true;
    const double muNewL = APPLY ? L.A[cLA].muNew : 0.0, muNewR = APPLY ? L.A[cRA].muNew : 0.0;
    const int binBL = STATS ? (int)L.S[cLS].binB : -1, binBR = STATS ? (int)L.S[cRS].binB : -1;
    int curA[F_PF][4], curS[F_PF][4];      // node reached while still routing, -1 once settled
    bool any = false;
#pragma unroll
    for (int j = 0; j < F_PF; ++j) {
      const int64_t qd = q0 + (int64_t)j * stride;
      const int valid = qd < nQuads ? ((a.n - (qd << 2)) >= 4 ? 4 : (int)(a.n - (qd << 2))) : 0;
      const unsigned pl[4] = {P.pl4[j].x, P.pl4[j].y, P.pl4[j].z, P.pl4[j].w};
      const unsigned lf[4] = {P.lf4[j].x, P.lf4[j].y, P.lf4[j].z, P.lf4[j].w};
      const unsigned xsv[4] = {xs[j].x, xs[j].y, xs[j].z, xs[j].w};
      const unsigned xav[4] = {xa[j].x, xa[j].y, xa[j].z, xa[j].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool ok = e < valid;
        nlA[j][e] = ok ? pl[e] : 0u; ndS[j][e] = -1; curA[j][e] = -1; curS[j][e] = -1;
        muOldV[j][e] = 0.0; muNewV[j][e] = 0.0; muS[j][e] = 0.0; binAV[j][e] = -1; binBV[j][e] = -1;
        // branch-free: every LDS read is unconditional (valid index either way), so that all reads of the thread's
        // observations are in flight together instead of one wait per divergent region
        if (APPLY) {
          const unsigned l = ok ? pl[e] : 0u;
          const d2_t rec = *reinterpret_cast<const d2_t*>(&L.A[l]);   // {old value, new value} of the observation's present leaf
          muOldV[j][e] = rec.x;
          const int ain = L.Ain[l];
          const bool goL = xav[e] <= (unsigned)rootCutA;
          const int child = goL ? cLA : cRA;
          const bool childLeaf = goL ? leafLA : leafRA;
          const bool routed = prevAcc && ok && ain != 0;
          curA[j][e] = (routed && !childLeaf) ? child : -1;
          nlA[j][e] = (routed && childLeaf) ? (unsigned)child : l;
          muNewV[j][e] = (routed && childLeaf) ? (goL ? muNewL : muNewR) : rec.y;
          any |= routed && !childLeaf;
        }
        if (STATS) {
          const i4_t rec = *reinterpret_cast<const i4_t*>(&L.S[ok ? lf[e] : 0u]);   // {mu lo, mu hi, binA | binB << 16, insub | pad << 16}
          muS[j][e] = __hiloint2double(rec.y, rec.x);
          binAV[j][e] = ok ? (int)(short)(rec.z & 0xffff) : -1;
          const bool goL = xsv[e] <= (unsigned)rootCutS;
          const int child = goL ? cLS : cRS;
          const bool childLeaf = goL ? leafLS : leafRS;
          const bool routed = ok && (rec.w & 0xffff) != 0;
          curS[j][e] = (routed && !childLeaf) ? child : -1;
          ndS[j][e] = (routed && childLeaf) ? child : -1;
          binBV[j][e] = (routed && childLeaf) ? (goL ? binBL : binBR) : -1;
          any |= routed && !childLeaf;
        }
      }
    }
    S4B_PASS_T(14);
    bool second = F_SECOND;
    int levels = 0;
    while (any) {   // deeper levels
      if (++levels > 2 * S4B_MAX_DEPTH) {     // (a walk that never reaches a leaf: tables that do not describe a tree — never hang the device)
        *a.errFlag |= S4B_ERR_INTERNAL | S4B_ERR_I_WAIT;
#ifdef S4B_TUNING
        if ((threadIdx.x & 63) == 0) { g_dbgSpin[0] = -(int)__LINE__; g_dbgSpin[1] = (curA[0][0] & 0xff) | ((curS[0][0] & 0xff) << 8) | (root << 16); g_dbgSpin[2] = (int)blockIdx.x; g_dbgSpin[3] = (int)threadIdx.x; }
#endif
        break;
      }
#ifdef S4B_CONTROL_TIMING
      if (APPLY && STATS && (int)blockIdx.x == S4B_TIMED_WG && threadIdx.x == 3 * 64) atomicAdd(&g_step[6], 1ull);
#endif
      unsigned xv[2][F_PF][4];
      if (second) {   // the cursors sit on a child of the root: its column is already here
#pragma unroll
        for (int j = 0; j < F_PF; ++j) {
          const unsigned sl[4] = {xs2[0][j].x, xs2[0][j].y, xs2[0][j].z, xs2[0][j].w}, sr[4] = {xs2[1][j].x, xs2[1][j].y, xs2[1][j].z, xs2[1][j].w};
          const unsigned al[4] = {xa2[0][j].x, xa2[0][j].y, xa2[0][j].z, xa2[0][j].w}, ar[4] = {xa2[1][j].x, xa2[1][j].y, xa2[1][j].z, xa2[1][j].w};
#pragma unroll
          for (int e = 0; e < 4; ++e) { xv[0][j][e] = curA[j][e] == rootLA ? al[e] : ar[e]; xv[1][j][e] = curS[j][e] == rootLS ? sl[e] : sr[e]; }
        }
      } else {
#pragma unroll
      for (int j = 0; j < F_PF; ++j) {
        const int64_t i0 = (q0 + (int64_t)j * stride) << 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          // unconditional loads (an inactive cursor reads column 0 at its own observation: valid and cached), all in flight together
          xv[0][j][e] = 0u; xv[1][j][e] = 0u;
          const int64_t ie = (i0 + e) < a.npad ? (i0 + e) : 0;
          if (APPLY) { const int v = curA[j][e] >= 0 ? (int)L.AP[curA[j][e]].var : 0; xv[0][j][e] = a.xbin[(size_t)(v >= 0 ? v : 0) * a.npad + (size_t)ie]; }
          if (STATS) { const int v = curS[j][e] >= 0 ? (int)L.SP[curS[j][e]].var : 0; xv[1][j][e] = a.xbin[(size_t)(v >= 0 ? v : 0) * a.npad + (size_t)ie]; }
        }
      }
      }
      second = false;
      any = false;
#pragma unroll
      for (int j = 0; j < F_PF; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (APPLY && curA[j][e] >= 0) {
            const NodeP p = L.AP[curA[j][e]];
            const int nd = (xv[0][j][e] <= (unsigned)p.cut) ? p.left : p.right;
            if (L.AP[nd].var >= 0) { curA[j][e] = nd; any = true; } else { curA[j][e] = -1; nlA[j][e] = (unsigned)nd; muNewV[j][e] = L.A[nd].muNew; }
          }
          if (STATS && curS[j][e] >= 0) {
            const NodeP p = L.SP[curS[j][e]];
            const int nd = (xv[1][j][e] <= (unsigned)p.cut) ? p.left : p.right;
            if (L.SP[nd].var >= 0) { curS[j][e] = nd; any = true; } else { curS[j][e] = -1; ndS[j][e] = nd; binBV[j][e] = (int)L.S[nd].binB; }
          }
        }
      }
    }
    S4B_PASS_T(15);
    // arithmetic
#pragma unroll
    for (int j = 0; j < F_PF; ++j) {
      const int64_t qd = q0 + (int64_t)j * stride;
      if (qd < nQuads) {
        const int64_t i0 = qd << 2;
        const int valid = (a.n - i0) >= 4 ? 4 : (int)(a.n - i0);
        double rr[4] = {P.r01[j].x, P.r01[j].y, P.r23[j].x, P.r23[j].y};
        const double ww[4] = {WEIGHTED ? P.w01[WEIGHTED ? j : 0].x : 1.0, WEIGHTED ? P.w01[WEIGHTED ? j : 0].y : 1.0,
                              WEIGHTED ? P.w23[WEIGHTED ? j : 0].x : 1.0, WEIGHTED ? P.w23[WEIGHTED ? j : 0].y : 1.0};
        if (APPLY) {
#pragma unroll
          for (int e = 0; e < 4; ++e) rr[e] = (rr[e] + muOldV[j][e]) - muNewV[j][e];
          store_r(R + i0, rr[0], rr[1]); store_r(R + i0 + 2, rr[2], rr[3]);
          if (prevAcc) { us4_t o4; o4.x = (unsigned short)nlA[j][0]; o4.y = (unsigned short)nlA[j][1]; o4.z = (unsigned short)nlA[j][2]; o4.w = (unsigned short)nlA[j][3];
                         __builtin_nontemporal_store(o4, reinterpret_cast<us4_t*>(prevPlane + i0)); }
        }
        if (STATS) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const bool ok = e < valid;
            const double r0 = WEIGHTED ? (rr[e] + muS[j][e]) * ww[e] : rr[e] + muS[j][e];
            const double r = ok ? r0 : 0.0;
            const int ba = binAV[j][e] >= 0 ? binAV[j][e] - base : -1;
            const int bb = ndS[j][e] >= 0 ? binBV[j][e] - base : -1 - base;
#pragma unroll
            for (int k = 0; k < NB; ++k) {
              const bool m = (ba == k) | (bb == k);
              const double md = __hiloint2double(m ? 0x3ff00000 : 0, 0);
              accS[k] = fma(md, r, accS[k]);
              accC[k] += md;
              if (WEIGHTED) accW[k] = fma(md, ww[e], accW[k]);
            }
          }
        }
      }
    }
    qStart = q0 + (int64_t)F_PF * stride;
  }
  {   // remaining quads: two requests in flight per thread
    struct Quad { double2 r01, r23; us4_t lf4, pl4, xs4, xa4; double2 w01, w23; };
    auto fetch = [&](int64_t q, Quad& o) {
      if (q < nQuads) {
        const int64_t i0 = q << 2;
        if (STATS && rootVarS >= 0) o.xs4 = *reinterpret_cast<const us4_t*>(colS + i0);
        if (APPLY && rootVarA >= 0) o.xa4 = *reinterpret_cast<const us4_t*>(colA + i0);
        if (APPLY) { o.r01 = *reinterpret_cast<const double2*>(R + i0); o.r23 = *reinterpret_cast<const double2*>(R + i0 + 2); }
        else {
          // a further bin pass of the same launch reads back what the first pass stored written-through (store_r): past this compute
          // unit's vector cache, which may still hold sectors of the line as they were loaded before the store (seen on the streaming
          // variant of the persistent sweep, round 5: 8 bytes of every 32 in the last 128 of each 512-byte block came back stale)
          o.r01.x = __hip_atomic_load(R + i0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); o.r01.y = __hip_atomic_load(R + i0 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          o.r23.x = __hip_atomic_load(R + i0 + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); o.r23.y = __hip_atomic_load(R + i0 + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (WEIGHTED) { o.w01 = *reinterpret_cast<const double2*>(W + i0); o.w23 = *reinterpret_cast<const double2*>(W + i0 + 2); }
        if (STATS) o.lf4 = __builtin_nontemporal_load(reinterpret_cast<const us4_t*>(leafPlane + i0));
        if (APPLY) o.pl4 = __builtin_nontemporal_load(reinterpret_cast<const us4_t*>(prevPlane + i0));
      }
    };
    Quad qa, qb;
    qa.w01 = qa.w23 = qb.w01 = qb.w23 = one2;
    qa.xs4 = qa.xa4 = qb.xs4 = qb.xa4 = zero4; qa.lf4 = qa.pl4 = qb.lf4 = qb.pl4 = zero4;
    int64_t qd = qStart;
    fetch(qd, qa); fetch(qd + stride, qb);
    for (; qd < nQuads; qd += stride) {
      const Quad c = qa;
      qa = qb;
      fetch(qd + 2 * stride, qb);
      process(qd, c.r01, c.r23, c.lf4, c.pl4, c.xs4, c.xa4, c.w01, c.w23);
    }
  }
  S4B_PASS_T(12);
  if (!STATS) return;
  // block reduction, fixed order: transposed halving inside each wave, then waves 0..7 in order (the control waves add zeros)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int accN[NB];   // the counts are small integers: their exchanges move one word instead of two
#pragma unroll
  for (int k = 0; k < NB; ++k) accN[k] = (int)accC[k];
  wave_sum_bins<NB>(accS, lane);
  wave_sum_bins<NB>(accN, lane);
  if (WEIGHTED) wave_sum_bins<WEIGHTED ? NB : 1>(accW, lane);
  if ((lane & (64 / NB - 1)) == 0) { const int k = wave_bin_of_lane<NB>(lane); L.redS[wv * NBMAX + k] = accS[0]; L.redN[wv * NBMAX + k] = accN[0];
                                     if (WEIGHTED) L.redW[wv * NBMAX + k] = accW[0]; }
  __syncthreads();
  if ((int)threadIdx.x < NB && base + (int)threadIdx.x < nbTotal) {
    const int k = threadIdx.x;
    double s = L.redS[k]; int c = L.redN[k]; double w = WEIGHTED ? L.redW[k] : 0.0;
#pragma unroll
    for (int v = 1; v < FBLOCK / 64; ++v) { s += L.redS[v * NBMAX + k]; c += L.redN[v * NBMAX + k]; if (WEIGHTED) w += L.redW[v * NBMAX + k]; }
    const size_t kind = (size_t)a.binCap * a.gridF;
    part[(size_t)(base + k) * a.gridF + blockIdx.x] = s;
    part[kind + (size_t)(base + k) * a.gridF + blockIdx.x] = (double)c;
    if (WEIGHTED) part[2 * kind + (size_t)(base + k) * a.gridF + blockIdx.x] = w;
  }
  // (no barrier here: a further bin pass of the same launch synchronises before it reuses the reduction slots — see the callers)
  S4B_PASS_T(13);
}

// (k_step's wave-register control code is compiled without the weighted predictor choice: with cgm(split.probs) every control step of a k_step launch is the
// sequential one of its tail — k_step then only finishes sweeps that k_sweep_sp handed over)
__device__ __forceinline__ bool step_fits_wave_k(const BartArrays& a, int need, int nb, int nc) { return step_fits_wave(need, nb, nc) && a.model.splitProbs == nullptr; }

// first launch of a sweep (one workgroup): tree 0 too large for the wave path -> propose it here on the global arrays
__global__ __launch_bounds__(FBLOCK) void k_step_pre(BartArrays a) {
  __shared__ double scratch[S4B_MAX_DEPTH];
  const int hwm0 = a.hwm[0];
  const bool big = !step_fits_wave_k(a, hwm0 + 2, 0, a.nc);
  if (threadIdx.x == 0) { *a.ticket = 0; a.preDone[0] = big ? 1 : 0; a.preDone[1] = 0; }
  if (!big) return;
  for (int i = threadIdx.x; i < (int)(sizeof(MTState) / 4); i += blockDim.x) ((uint32_t*)&a.rngF[1])[i] = ((const uint32_t*)&a.rngF[0])[i];
  __syncthreads();
  if (threadIdx.x == 0) { BartArrays b = a; b.rng = a.rngF + 1; b.rng->pad = 0; control_global_path(b, -1, 0, scratch); }
  __syncthreads();
  snapshot_from_main(a, 0);
}

#ifdef S4B_TUNING
__device__ int g_dbgMark;
__device__ int g_prog[640 * 8];
#define S4B_CP(n) do { if ((threadIdx.x & 63) == 0) g_prog[blockIdx.x * 8 + (threadIdx.x >> 6)] = (t << 8) | (n); } while (0)
#else
#define S4B_CP(n)
#endif
template <bool WEIGHTED>
__global__ __launch_bounds__(FBLOCK) void k_step(BartArrays a, int t) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ ControlShared S;
  __shared__ StepShared F;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nc = a.nc;
  const bool doDecide = t > 0, doPropose = t < a.T;
  const int tt = doDecide ? t - 1 : 0, tn = doPropose ? t : 0;
  const int tnn = t + 1 < a.T ? t + 1 : tn;                // tree after tn (its slot count decides how the NEXT launch runs)
  const StepScratch& cT = a.sc[tt & 1];
  const StepScratch& cN = a.sc[tn & 1];
  const StepLds L = carve_step(smem, nc);
  const bool first = blockIdx.x == 0;
  // the LAST workgroup owns no observations: it decides like the others, writes the results back and then draws the proposals
  // of the tree after next while the others run the pass
  const bool ctl = (int)blockIdx.x == (int)gridDim.x - 1;
#ifdef S4B_LIGHT_TIMING
  const long long tL0 = wall_clock64(); long long tArr = tL0;
#endif
#ifdef S4B_CONTROL_TIMING
  const long long tq0 = wall_clock64();
  if (threadIdx.x == 0 && doDecide && doPropose && (int)blockIdx.x == S4B_TIMED_WG) atomicAdd(&g_step[0], 1ull);
  if (threadIdx.x == 0 && doDecide && doPropose) atomicAdd(&g_wgS[blockIdx.x], (unsigned long long)tq0);
#endif
  double* const partIn = a.partF + (size_t)((t + 1) & 1) * 3 * a.binCap * a.gridF;    // statistics of tree t-1 (written by launch t-1)
  double* const partOut = a.partF + (size_t)(t & 1) * 3 * a.binCap * a.gridF;
  const size_t kindStride = (size_t)a.binCap * a.gridF;
  if (threadIdx.x == 0) { S.arrived = 0; S.verdict = 0; F.needBig = 0; F.prevAcc = 0; F.prevRoot = 0; F.hp = 0; F.root = 0; F.nb = 0; F.hwmS = 0; F.last = 0; F.sset = 0; F.paGo = 0; F.paType = 0; F.paStatus = 0; F.paNbA = 0; }
  const int pre = __builtin_amdgcn_readfirstlane(a.preDone[t & 1]);
  if (first && threadIdx.x == 0) a.preDone[(t + 1) & 1] = 0;   // nobody reads that slot in this launch; its tail may raise it
  __syncthreads();
  S4B_CP(1);

  const bool isPass = wv >= 3;
  const int64_t nQuads = (a.n + 3) >> 2;
  const int64_t stride = (int64_t)((int)gridDim.x - 1) * F_PT;     // the pass workgroups: all but the last
  const int64_t q0 = (int64_t)blockIdx.x * F_PT + threadIdx.x;
  const int lt = (int)threadIdx.x - F_CTL;                    // loader index of a thread of waves 3-7
  const uint16_t* __restrict__ leafPlaneS = a.leaf + (size_t)tn * a.npad;
  const uint16_t* __restrict__ leafPlaneA = a.leaf + (size_t)tt * a.npad;
  // the first F_PF quads of every thread are requested before the control code runs (nothing of them depends on the pending
  // decision): own quads into P; the loader threads also request the quads of the control threads (H) and hand them over
  StepPre<WEIGHTED> P, H;
  auto request = [&](StepPre<WEIGHTED>& o, int64_t first) {
#pragma unroll
    for (int j = 0; j < F_PF; ++j) {
      const int64_t qd = first + (int64_t)j * stride;
      if (qd < nQuads) {
        const int64_t i0 = qd << 2;
        o.r01[j] = *reinterpret_cast<const double2*>(a.R + i0); o.r23[j] = *reinterpret_cast<const double2*>(a.R + i0 + 2);
        if (WEIGHTED) { o.w01[WEIGHTED ? j : 0] = *reinterpret_cast<const double2*>(a.wts + i0); o.w23[WEIGHTED ? j : 0] = *reinterpret_cast<const double2*>(a.wts + i0 + 2); }
        if (doPropose) o.lf4[j] = __builtin_nontemporal_load(reinterpret_cast<const us4_t*>(leafPlaneS + i0));
        if (doDecide) o.pl4[j] = __builtin_nontemporal_load(reinterpret_cast<const us4_t*>(leafPlaneA + i0));
      }
    }
  };
  auto prefetch = [&]() {
    request(P, q0);
    if (!pre && lt < F_CTL) request(H, (int64_t)blockIdx.x * F_PT + lt);
  };
  auto handOver = [&]() {   // loader thread lt -> control thread lt, through LDS
    if (pre || lt >= F_CTL) return;
#pragma unroll
    for (int j = 0; j < F_PF; ++j) {
      const int sl = j * F_CTL + lt;
      L.hR01[sl] = H.r01[j]; L.hR23[sl] = H.r23[j]; L.hLf[sl] = H.lf4[j]; L.hPl[sl] = H.pl4[j];
      if (WEIGHTED) { L.hW01[sl] = H.w01[WEIGHTED ? j : 0]; L.hW23[sl] = H.w23[WEIGHTED ? j : 0]; }
    }
  };
  // control already done by the previous launch's tail: stage the pass tables from global memory (what k_tree does)
  auto stagePre = [&]() {
    if (doPropose) {
      const Proposal pr = cN.head->pr;
      const double* muS = a.mu + (size_t)tn * nc;
      for (int i = threadIdx.x; i < pr.hwm; i += FBLOCK) {
        NodeS s; s.mu = muS[i]; s.binA = cN.binA[i]; s.binB = cN.binB[i]; s.insub = cN.insub[i]; s.pad = 0;
        NodeP p; p.var = cN.pvar[i]; p.cut = cN.pcut[i]; p.left = cN.pleft[i]; p.right = cN.pright[i];
        L.S[i] = s; L.SP[i] = p;
      }
      if (threadIdx.x == 0) {
        F.root = pr.node; F.nb = pr.nbA + pr.nbB; F.hwmS = pr.hwm;
        const int hwmN = a.hwm[tn];
        int needNext = pr.hwm > hwmN ? pr.hwm : hwmN;
        if (t + 1 < a.T && a.hwm[tnn] + 2 > needNext) needNext = a.hwm[tnn] + 2;
        F.needBig = step_fits_wave_k(a, needNext, pr.nbA + pr.nbB, nc) ? 0 : 1;
      }
    }
    if (doDecide) {
      const int hp = cT.head->pr.hwm > a.hwm[tt] ? cT.head->pr.hwm : a.hwm[tt];
      const size_t o = (size_t)tt * nc;
      for (int i = threadIdx.x; i < hp; i += FBLOCK) {
        NodeA q; q.muOld = cT.muOld[i]; q.muNew = a.mu[o + i];
        NodeP p; p.var = a.var[o + i]; p.cut = a.cut[o + i]; p.left = a.left[o + i]; p.right = a.right[o + i];
        L.A[i] = q; L.AP[i] = p; L.Ain[i] = cT.insub[i];
      }
      if (threadIdx.x == 0) { F.prevAcc = *cT.accepted; F.prevRoot = cT.head->pr.node; F.hp = hp; }
    }
  };
  if (isPass) {
    // ================================================================ reducers: partials of statistics(t-1) -> bin totals
    if (doDecide && !pre) {
      const int redIdx = wv - 3;
      const int ridx = redIdx * 64 + lane;
      constexpr int RT = C_NRED * 64;
      const int grid = a.gridF;
      double pv[16], qv[16];
      const int b0 = ridx, b1 = ridx + RT;
      const bool in0 = b0 < grid, in1 = b1 < grid;
      const size_t c0 = in0 ? b0 : 0, c1 = in1 ? b1 : 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) { pv[j] = partIn[(size_t)j * grid + c0]; pv[8 + j] = partIn[kindStride + (size_t)j * grid + c0]; }
      // (the partials are 32 KB per workgroup, requested by every CU at the same moment as the control data of waves 0-2, through
      // the same memory pipeline: every request saved here shortens the wait of wave 0)
      const bool two = grid > RT;     // more partial columns than reducer lanes (only with an oversized grid): a second one per lane
      if (two) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { qv[j] = partIn[(size_t)j * grid + c1]; qv[8 + j] = partIn[kindStride + (size_t)j * grid + c1]; }
      }
      const int nbAll = cT.head->pr.nbA + cT.head->pr.nbB;
      if (two) {
#pragma unroll
        for (int j = 0; j < 16; ++j) pv[j] = (in0 ? pv[j] : 0.0) + (in1 ? qv[j] : 0.0);
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) pv[j] = in0 ? pv[j] : 0.0;
      }
      wave_sum_bins<16>(pv, lane);
      if ((lane & 3) == 0) { const int k = wave_bin_of_lane<16>(lane); S.red[k >> 3][redIdx][k & 7] = pv[0]; }
      if (WEIGHTED) {
        double wv8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) wv8[j] = 0.0;
        for (int b = ridx; b < grid; b += RT) {
#pragma unroll
          for (int j = 0; j < 8; ++j) wv8[j] += partIn[2 * kindStride + (size_t)j * grid + b];
        }
        wave_sum_bins<8>(wv8, lane);
        if ((lane & 7) == 0) S.red[2][redIdx][wave_bin_of_lane<8>(lane)] = wv8[0];
      }
      for (int k = 8; k < nbAll && k < 64; ++k) {   // rare: more than 8 bins
        double sm = 0.0, c = 0.0, wt = 0.0;
        for (int b = ridx; b < grid; b += RT) { sm += partIn[(size_t)k * grid + b]; c += partIn[kindStride + (size_t)k * grid + b]; if (WEIGHTED) wt += partIn[2 * kindStride + (size_t)k * grid + b]; }
        sm = wave_sum(sm); c = wave_sum(c); wt = wave_sum(wt);
        if (lane == 0) { S.red[0][redIdx][k] = sm; S.red[1][redIdx][k] = c; S.red[2][redIdx][k] = wt; }
      }
      if (lane == 0) __hip_atomic_fetch_add(&S.arrived, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (lane == 0 && wv == 3) S4B_STEP_T(1);
      // the observations only now: the totals are on the critical path (a wait on the partials would otherwise also wait
      // for these requests), the observations are needed after the barrier, several microseconds from here
      if (!ctl) prefetch();
    } else if (!ctl) prefetch();
    if (!ctl) handOver();
    if (pre) stagePre();
    if (ctl && doPropose && !pre && wv <= 4) {
      // control workgroup: once the proposal of tree tn is settled, what the image of the winner holds becomes scratch set tn & 1
      // (wave 3) and the generator state it leaves behind the stream of the next launch (wave 4); a proposal drawn by wave 0 in
      // this launch is written back by wave 0 itself
      spin_until(&F.paGo, 1, a.errFlag);
      const int wslot = __builtin_amdgcn_readfirstlane(F.sset);
      if (wslot >= 1 && wv == 3) {
        const CandSet cw = cand_view(a, t & 1, wslot - 1);
        for (int i = lane; i < nc; i += 64) {
          int16_t row[SF_COUNT];
#pragma unroll
          for (int r = 0; r < SF_COUNT; ++r) row[r] = cw.slab[r * nc + i];
          const uint8_t ins = cw.insub[i]; const double sm = cw.snapMu[i]; const int32_t sc = cw.snapCnt[i];
#pragma unroll
          for (int r = 0; r < SF_COUNT; ++r) cN.slab[r * nc + i] = row[r];
          cN.insub[i] = ins; cN.snapMu[i] = sm; cN.snapCnt[i] = sc;
        }
        if (lane < 28) ((int32_t*)cN.head)[lane] = ((const int32_t*)cw.head)[lane];
      }
      if (wslot >= 1 && wv == 4) {
        constexpr int MTW = (int)(sizeof(MTState) / 4), MTJ = (MTW + 63) / 64;
        MTState* rngOut = a.rngF + ((t + 1) & 1);
#pragma unroll
        for (int j = 0; j < MTJ; ++j) { const int i = lane + j * 64; if (i < MTW) ((uint32_t*)rngOut)[i] = ((const uint32_t*)&S.rng[wslot])[i]; }
      }
    }
    if (lane == 0 && wv == 3) S4B_STEP_T(16);
    S4B_ARRIVE();
    __syncthreads();
  } else if (pre) {
    if (!ctl) request(P, q0);
    stagePre();
    // no proposal is drawn ahead in a launch whose control step ran on the global-memory path: the next launch proposes itself
    if (ctl && threadIdx.x == 0 && doPropose && t + 1 < a.T) { cand_view(a, (t + 1) & 1, 0).meta[0] = 0; cand_view(a, (t + 1) & 1, 1).meta[0] = 0; }
    __syncthreads();
  } else {
    // ================================================================ decider (wave 0) and candidate waves (1, 2)
    // Wave 0 decides tree t-1.  The proposal of tree t was drawn during the previous launch, once per number of draws that decision
    // can consume (two images in global memory): waves 1, 2 fetch one image each, stage its tables and wait for the verdict.  In
    // the control workgroup they then draw the two images of tree t+1 while the other workgroups run the pass, so that no
    // proposal is drawn on the critical path (only at the start of a sweep, after a step on the global-memory path, or when
    // neither image fits the draws actually consumed, wave 0 proposes itself, as before).
    const bool isDecider = wv == 0;
    if (isDecider && lane == 0) S4B_STEP_T(30);
    const int candIdx = isDecider ? 0 : wv - 1;
    const int slot = isDecider ? 0 : 1 + candIdx;
    bool didDecide = false, ownProp = false; int dHwmNew = 0, dCntOut = 0, pPerr = 0, pCntOut = 0, wbRngSlot = -1; int32_t dAccepted = 0;
    StepRecord dRec; dRec.type = 0; dRec.status = 0; dRec.var = 0; dRec.split = 0; dRec.numLeaves = 0;
    Proposal pPr; pPr.type = 0; pPr.status = 0; pPr.node = 0; pPr.var = 0; pPr.split = 0; pPr.nbA = 0; pPr.nbB = 0; pPr.hwm = 0; pPr.newLeft = 0; pPr.newRight = 0;
    pPr.pad0 = 0; pPr.pad1 = 0; pPr.priorRatio = 0; pPr.transRatio = 0; pPr.XLogPi = 0; pPr.YLogPi = 0;
    const size_t oT = (size_t)tt * nc, oN = (size_t)tn * nc, oNN = (size_t)tnn * nc;
    const bool laneIn = lane < nc;
    const unsigned li = laneIn ? (unsigned)lane : 0u;   // unsigned: uniform row base + 32-bit lane offset is one address mode
    int16_t* const tI = a.treeI16; const size_t ts = (size_t)a.T * nc; int32_t* const tS = a.treeI32; const size_t tT = (size_t)a.T;
    int16_t* const sT = cT.slab; int16_t* const sN = cN.slab;
    const MTState* rngIn = a.rngF + (t & 1);
    MTState* rngOut = a.rngF + ((t + 1) & 1);
    const bool spec = doDecide && doPropose;
    const bool ahead = doPropose && t + 1 < a.T;          // this launch draws the images of tree t+1
    const bool drawsAhead = !isDecider && ctl && ahead;   // ... in these two waves
    const CandSet cdIn = cand_view(a, t & 1, candIdx);
    // ---- one hop: everything this wave needs
    WaveModel m;
    static_cast<ModelView&>(m) = a.model;
    m.scratch = S.scratch[slot];
    constexpr int MTW = (int)(sizeof(MTState) / 4), MTJ = (MTW + 63) / 64;
    uint32_t mtw[MTJ];
    const bool wantRng = isDecider || (ctl && spec);      // wave 0: the stream as the previous launch left it; control workgroup: what each image leaves behind
    const bool wantModel = isDecider || drawsAhead;
    // the tree this wave may propose for: wave 0 tree tn (only when it has to), waves 1, 2 tree tnn (used in the control workgroup)
    WaveTree curN; WaveCache caN; WaveTables tbN; WaveArrD muN; int cntN = 0;
    curN.nc = nc < 64 ? nc : 64;
    muN.load(0.0);
    auto loadTree = [&](size_t o) {   // from the main arrays (no launch writes them while it reads them)
      // (nothing here looks at what it requests: a use would wait for everything requested before it)
      curN.var.r = (int)(tI + TF_VAR * ts + o)[li]; curN.cut.r = ((const uint16_t*)(tI + TF_CUT * ts + o))[li]; curN.left.r = (tI + TF_LEFT * ts + o)[li];
      curN.right.r = (tI + TF_RIGHT * ts + o)[li]; curN.parent.r = (tI + TF_PARENT * ts + o)[li]; curN.na.r = (tI + TF_NA * ts + o)[li];
      curN.dep.r = (tI + TF_DEP * ts + o)[li];
      caN.leaf.r = (tI + TF_LEAF * ts + o)[li]; caN.pre.r = (tI + TF_PRE * ts + o)[li]; caN.post.r = (tI + TF_POST * ts + o)[li];
      muN.load(a.mu[o + li]); cntN = a.cnt[o + li];
    };
    const bool treeEarly = !isDecider || !doDecide;
    // the image of this wave's candidate: the tables of the pass
    int iVar = 0, iCut = 0, iLeft = 0, iRight = 0, iBinA = 0, iBinB = 0, iInsub = 0; WaveArrD iMu; iMu.load(0.0);
    if (!isDecider) {
      const int16_t* sI = cdIn.slab;
      iVar = (sI + SF_VAR * nc)[li]; iCut = ((const uint16_t*)(sI + SF_CUT * nc))[li]; iLeft = (sI + SF_LEFT * nc)[li]; iRight = (sI + SF_RIGHT * nc)[li];
      iBinA = (sI + SF_BINA * nc)[li]; iBinB = (sI + SF_BINB * nc)[li]; iInsub = cdIn.insub[li]; iMu.load(cdIn.snapMu[li]);
    }
    WaveTree curT; WaveTables tbT; WaveCache caT; WaveArrD mu, muOld; WaveArr<int32_t> cnt;
    if (isDecider && doDecide) {   // snapshot of tree tt + its pending proposal, all from scratch set tt & 1
      curT.var.r = (sT + SF_CVAR * nc)[li]; curT.cut.r = ((const uint16_t*)(sT + SF_CCUT * nc))[li]; curT.left.r = (sT + SF_CLEFT * nc)[li];
      curT.right.r = (sT + SF_CRIGHT * nc)[li]; curT.parent.r = (sT + SF_CPARENT * nc)[li]; curT.na.r = (sT + SF_CNA * nc)[li];
      curT.dep.r = (sT + SF_CDEP * nc)[li]; curT.nc = curN.nc;
      tbT.prop.var.r = (sT + SF_VAR * nc)[li]; tbT.prop.cut.r = ((const uint16_t*)(sT + SF_CUT * nc))[li]; tbT.prop.left.r = (sT + SF_LEFT * nc)[li];
      tbT.prop.right.r = (sT + SF_RIGHT * nc)[li]; tbT.prop.parent.r = (sT + SF_PARENT * nc)[li]; tbT.prop.na.r = (sT + SF_NA * nc)[li];
      tbT.prop.dep.r = (sT + SF_DEP * nc)[li]; tbT.prop.nc = curN.nc;
      tbT.binA.r = (sT + SF_BINA * nc)[li]; tbT.binB.r = (sT + SF_BINB * nc)[li]; tbT.insub.r = cT.insub[li]; tbT.list.r = 0;
      caT.leaf.r = (sT + SF_CLEAF * nc)[li]; caT.pre.r = (sT + SF_CPRE * nc)[li]; caT.post.r = (sT + SF_CPOST * nc)[li];
      mu.load(cT.snapMu[li]); muOld.load(0.0); cnt.r = cT.snapCnt[li];
    }
    // scalars: wave 0 {pending proposal of tt, per-tree scalars of tn, slots of tnn}; waves 1, 2 {proposal of their image + the
    // scalars of tree tn it was drawn from, per-tree scalars of tnn}
    StepScalars g;
    step_header_load(g, a, isDecider ? cT.head : cdIn.head, isDecider ? tn : tnn, tnn, lane);
    // meta words of the images: wave 0 {valid, draws} of both, waves 1, 2 {valid, draws, propose() error} of their own
    int metaW;
    {
      const int32_t* m0 = cand_view(a, t & 1, 0).meta; const int32_t* m1 = cand_view(a, t & 1, 1).meta;
      const int32_t* mp = isDecider ? ((lane & 2) ? m1 : m0) + (lane & 1) : cdIn.meta + (lane < 3 ? lane : 0);
      metaW = *mp;
    }
    // (requested after what decide() needs first: wave 0 enters decide() as soon as the scalars, the snapshot and the totals are there;
    // the generator is first needed at the accept test, the prior tables only by a wave that proposes or keeps the cache)
    // (every request below is unconditional wherever its address is valid anyway: a request under a condition is a branch, and
    // the compiler waits for everything in flight where branches join)
    {
      const uint32_t* src = isDecider ? (const uint32_t*)rngIn : (const uint32_t*)cdIn.rng;
#pragma unroll
      for (int j = 0; j < MTJ; ++j) { const int i = lane + j * 64; mtw[j] = src[i < MTW ? i : 0]; }
    }
    m.pg.load(a.model.pgDepth[lane]); m.lpg.load(a.model.logPg[lane]); m.l1pg.load(a.model.log1mPg[lane]);
    m.li0.load(a.model.logInt[lane < m.logIntLen ? lane : 0]); m.li1.load(a.model.logInt[64 + lane < m.logIntLen ? 64 + lane : 0]);
    m.nc0 = a.numCuts[lane < a.P ? lane : 0]; m.nc1 = a.numCuts[64 + lane < a.P ? 64 + lane : 0];
    if (treeEarly) loadTree(isDecider ? oN : oNN);
    // the drawing waves: proposal scalars {type, status, .., leaves} + valid flag of image 0 and the generator state it leaves behind
    // (requested last: they sit under a condition)
    int pa0W = 0; uint32_t mt0[MTJ];
#pragma unroll
    for (int j = 0; j < MTJ; ++j) mt0[j] = 0u;
    if (drawsAhead) {
      const CandSet c0 = cand_view(a, t & 1, 0);
      const int32_t* hp = lane == 8 ? c0.meta : (const int32_t*)c0.head + (lane < 8 ? lane : 0);
      pa0W = *hp;
#pragma unroll
      for (int j = 0; j < MTJ; ++j) { const int i = lane + j * 64; mt0[j] = ((const uint32_t*)c0.rng)[i < MTW ? i : 0]; }
    }
    if (isDecider && lane == 0) S4B_STEP_T(31);
    // ---- first uses (in the order of the requests: a use waits for everything requested before it)
    metaW = (spec && lane < 4) ? metaW : 0;
    bool lateReady = false;
    auto finishLoads = [&]() {   // generator words into LDS, prior tables masked to their lengths, (tree) free slots marked
      if (lateReady) return;
      lateReady = true;
      if (wantRng) {
#pragma unroll
        for (int j = 0; j < MTJ; ++j) { const int i = lane + j * 64; if (i < MTW) ((uint32_t*)&S.rng[slot])[i] = mtw[j]; }
      }
      m.li0.load(lane < m.logIntLen ? m.li0.mine() : 0.0); m.li1.load(64 + lane < m.logIntLen ? m.li1.mine() : 0.0);
      m.nc0 = lane < a.P ? m.nc0 : 0; m.nc1 = 64 + lane < a.P ? m.nc1 : 0;
      if (treeEarly) curN.var.r = laneIn ? curN.var.r : (int)NODE_FREE;
      if (drawsAhead) {
#pragma unroll
        for (int j = 0; j < MTJ; ++j) { const int i = lane + j * 64; if (i < MTW) ((uint32_t*)&F.rngB[candIdx])[i] = mt0[j]; }
      }
    };
    (void)wantModel;
    if (!isDecider) finishLoads();   // (wave 0 does this inside decide(), right before the first draw)
    if (isDecider && lane == 0) S4B_STEP_T(2);
    if (wv == 1 && lane == 0) S4B_STEP_T(19);
    if (isDecider) {
      Proposal prT; g.proposal(prT);
      if (!doDecide) { prT.type = MOVE_CHANGE; prT.status = -1; prT.nbA = 0; prT.nbB = 0; prT.hwm = 0; prT.node = 0; }
      const int hwmT = doDecide ? g.i32(20) : 0, hwmN = g.i32(40 + TI_HWM), hwmNN = g.i32(48);
      caN.nl = g.i32(40 + TI_NL); caN.ni = g.i32(40 + TI_NI); caN.g = g.i32(40 + TI_G); caN.gn = g.i32(40 + TI_GN); caN.valid = g.i32(40 + TI_VALID);
      caN.logPi = g.f64(1);
      int need = 0, nb = 0;
      if (doDecide) { need = prT.hwm > hwmT ? prT.hwm : hwmT; nb = prT.nbA + prT.nbB; }
      if (doPropose && hwmN + 2 > need) need = hwmN + 2;
      if (!step_fits_wave_k(a, need, nb, nc) && lane == 0) *a.errFlag |= S4B_ERR_INTERNAL;   // the previous launch should have taken this step over
      const int v0 = spec ? __builtin_amdgcn_readlane(metaW, 0) : 0, h0 = __builtin_amdgcn_readlane(metaW, 1);
      const int v1 = spec ? __builtin_amdgcn_readlane(metaW, 2) : 0, h1 = __builtin_amdgcn_readlane(metaW, 3);
      WaveRng rng; rng.st = &S.rng[0]; rng.mti = 0; rng.wbase = -64; rng.win = 0u; rng.count = 0; rng.regen = 0;
      auto openRng = [&]() { finishLoads(); rng.open(&S.rng[0]); };   // decide() calls this right before its first draw
      int winner = 0;
      if (!doDecide) openRng();
      if (doDecide) {
        caT.nl = g.i32(21); caT.ni = g.i32(22); caT.g = g.i32(23); caT.gn = g.i32(24); caT.valid = 1;
        caT.logPi = g.f64w(26);
        const double sigma = g.f64(2);
        spin_until(&S.arrived, C_NRED, a.errFlag);
        if (lane == 0) S4B_STEP_T(3);
        WaveArrD binSum, binCnt;
        {
          double sSum = 0.0, sCnt = 0.0;
          if (lane < nb) {
            sSum = S.red[0][0][lane]; sCnt = S.red[1][0][lane];
#pragma unroll
            for (int r = 1; r < C_NRED; ++r) { sSum += S.red[0][r][lane]; sCnt += S.red[1][r][lane]; }
          }
          binSum.load(sSum); binCnt.load(sCnt);
        }
        WaveArrD binWt = binCnt;
        if (WEIGHTED) {
          double sWt = 0.0;
          if (lane < nb) {
            sWt = S.red[2][0][lane];
#pragma unroll
            for (int r = 1; r < C_NRED; ++r) sWt += S.red[2][r][lane];
          }
          binWt.load(sWt);
        }
        DecideWork<WaveArrD> wk;
        wk.ll.load(0.0); wk.lc.load(0.0); wk.ls.load(0.0); wk.u1.load(0.5); wk.u2.load(0.5); wk.val.load(0.0); wk.lw.load(0.0);
        StepRecord rec; int32_t accepted = 0;
        auto post = [&]() {   // the draws are counted: which image (if any) was drawn from the position they leave behind?
          const int used = rng.count;
          winner = (v0 && used == h0) ? 1 : ((v1 && used == h1) ? 2 : 0);
          if (lane == 0) __hip_atomic_store(&S.verdict, winner ? winner : 3, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (lane == 0) S4B_STEP_T(23);
        };
        // (only the control workgroup writes the tree back: the others skip the upkeep of its structure cache)
        const int hwmNew = decide(curT, mu, cnt, muOld, hwmT, m, sigma, &rng, &prT, tbT, binCnt, binSum, binWt, wk, &accepted, &rec, caT, post, ctl, openRng);
        const int cntOut = prT.hwm > hwmNew ? prT.hwm : hwmNew;
        if (lane == 0) S4B_STEP_T(4);
        // apply half of the pass: tables straight from the registers
        if (lane < cntOut) {
          NodeA qa; qa.muOld = muOld.mine(); qa.muNew = mu.mine();
          NodeP pa; pa.var = (int16_t)curT.var.r; pa.cut = (uint16_t)curT.cut.r; pa.left = (int16_t)curT.left.r; pa.right = (int16_t)curT.right.r;
          L.A[lane] = qa; L.AP[lane] = pa; L.Ain[lane] = (uint8_t)tbT.insub.r;
        }
        if (lane == 0) { F.prevAcc = accepted; F.prevRoot = prT.node; F.hp = cntOut; }
        didDecide = true; dHwmNew = hwmNew; dCntOut = cntOut; dAccepted = accepted; dRec = rec;
      }
      if (lane == 0) S4B_STEP_T(5);
      if (!doPropose) { rng.close(); S.rng[0].pad = 0; wbRngSlot = 0; }
#ifdef S4B_CONTROL_TIMING
      if (spec && ctl && lane == 0) { atomicAdd(&g_step[29], 1ull); if (winner == 0) atomicAdd(&g_step[28], 1ull); }
#endif
      if (doPropose && winner == 0) {
        // ============================================================ proposal of tree tn, in this launch
        if (doDecide) { loadTree(oN); curN.var.r = laneIn ? curN.var.r : (int)NODE_FREE; }
        if (!caN.valid) tv_rebuild_cache(curN, m, caN);
        tbN.prop = curN;
        tbN.binA.r = -1; tbN.binB.r = -1; tbN.insub.r = 0; tbN.list.r = 0;
        Proposal prN;
        const int perr = propose(curN, hwmN, m, &rng, &prN, tbN, caN);
        if (lane < prN.hwm) {   // statistics half of the pass: table set 0, straight from the registers
          NodeS s; s.mu = muN.mine(); s.binA = (int16_t)tbN.binA.r; s.binB = (int16_t)tbN.binB.r; s.insub = (int16_t)tbN.insub.r; s.pad = 0;
          NodeP p; p.var = (int16_t)tbN.prop.var.r; p.cut = (uint16_t)tbN.prop.cut.r; p.left = (int16_t)tbN.prop.left.r; p.right = (int16_t)tbN.prop.right.r;
          L.S3[lane] = s; L.SP3[lane] = p;
        }
        const int cntOut = prN.hwm;
        // does the control step of the NEXT launch (decide tn, propose tnn) fit the wave path?
        int needNext = prN.hwm > hwmN ? prN.hwm : hwmN;
        if (t + 1 < a.T && hwmNN + 2 > needNext) needNext = hwmNN + 2;
        const int big = step_fits_wave(needNext, prN.nbA + prN.nbB, nc) ? 0 : 1;
        if (lane == 0) { F.root = prN.node; F.nb = prN.nbA + prN.nbB; F.hwmS = cntOut; F.needBig = big; F.sset = 0;
                         F.paType = prN.type; F.paStatus = prN.status; F.paNbA = prN.nbA; }
        ownProp = true; pPerr = perr; pCntOut = cntOut; pPr = prN;
        rng.close(); S.rng[0].pad = 0; wbRngSlot = 0;
        if (lane == 0) __hip_atomic_store(&F.paGo, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      // global write-backs (control workgroup only; nothing of this is read by anybody during this launch)
      if (ctl) {
        if (didDecide) {   // the decided tree goes to the main arrays (the other workgroups read its snapshot, never these)
          wave_tree_store(curT, tI + TF_VAR * ts + oT, (uint16_t*)(tI + TF_CUT * ts + oT), tI + TF_LEFT * ts + oT, tI + TF_RIGHT * ts + oT,
                          tI + TF_PARENT * ts + oT, dCntOut, lane);
          if (lane < dCntOut) { a.mu[oT + lane] = mu.mine(); a.cnt[oT + lane] = cnt.r; tI[TF_NA * ts + oT + lane] = (int16_t)curT.na.r; tI[TF_DEP * ts + oT + lane] = (int16_t)curT.dep.r; }
          if (laneIn) { tI[TF_LEAF * ts + oT + lane] = (int16_t)caT.leaf.r; tI[TF_PRE * ts + oT + lane] = (int16_t)caT.pre.r; tI[TF_POST * ts + oT + lane] = (int16_t)caT.post.r; }
          if (lane == 0) {
            tS[TI_HWM * tT + tt] = dHwmNew; tS[TI_NL * tT + tt] = caT.nl; tS[TI_NI * tT + tt] = caT.ni; tS[TI_G * tT + tt] = caT.g; tS[TI_GN * tT + tt] = caT.gn;
            tS[TI_VALID * tT + tt] = 1; a.clogpi[tt] = caT.logPi;
            *cT.accepted = dAccepted;
            if (a.traceOn) push_trace(a, dRec);
          }
        }
        if (ownProp) {
          if (pPerr != 0 && lane == 0) *a.errFlag |= S4B_ERR_NODE_CAPACITY;
          wave_tree_store(tbN.prop, sN + SF_VAR * nc, (uint16_t*)(sN + SF_CUT * nc), sN + SF_LEFT * nc, sN + SF_RIGHT * nc, sN + SF_PARENT * nc, pCntOut, lane);
          if (lane < pCntOut) { sN[SF_BINA * nc + lane] = (int16_t)tbN.binA.r; sN[SF_BINB * nc + lane] = (int16_t)tbN.binB.r; cN.insub[lane] = (uint8_t)tbN.insub.r;
                                sN[SF_NA * nc + lane] = (int16_t)tbN.prop.na.r; sN[SF_DEP * nc + lane] = (int16_t)tbN.prop.dep.r; }
          // snapshot of tree tn: what the next launch decides from
          if (laneIn) {
            sN[SF_CVAR * nc + lane] = (int16_t)curN.var.r; ((uint16_t*)sN)[SF_CCUT * nc + lane] = (uint16_t)curN.cut.r; sN[SF_CLEFT * nc + lane] = (int16_t)curN.left.r;
            sN[SF_CRIGHT * nc + lane] = (int16_t)curN.right.r; sN[SF_CPARENT * nc + lane] = (int16_t)curN.parent.r; sN[SF_CNA * nc + lane] = (int16_t)curN.na.r;
            sN[SF_CDEP * nc + lane] = (int16_t)curN.dep.r; sN[SF_CLEAF * nc + lane] = (int16_t)caN.leaf.r; sN[SF_CPRE * nc + lane] = (int16_t)caN.pre.r;
            sN[SF_CPOST * nc + lane] = (int16_t)caN.post.r; cN.snapMu[lane] = muN.mine(); cN.snapCnt[lane] = cntN;
          }
          step_header_store(pPr, hwmN, caN.nl, caN.ni, caN.g, caN.gn, caN.logPi, cN.head, lane);
        }
        if (wbRngSlot == 0) {   // the stream ends in this wave
#pragma unroll
          for (int j = 0; j < MTJ; ++j) { const int i = lane + j * 64; mtw[j] = ((const uint32_t*)&S.rng[0])[i < MTW ? i : 0]; }
#pragma unroll
          for (int j = 0; j < MTJ; ++j) { const int i = lane + j * 64; if (i < MTW) ((uint32_t*)rngOut)[i] = mtw[j]; }
        }
      }
      if (lane == 0) S4B_STEP_T(7);
    } else {
      // ============================================================== waves 1, 2
      Proposal prC; g.proposal(prC);
      const int hwmN = g.i32(20);                   // slots of tree tn when the image was drawn
      const int hwmNN = g.i32(40 + TI_HWM);         // slots of tree tnn
      const int valid = spec ? __builtin_amdgcn_readlane(metaW, 0) : 0;
      const int perrC = __builtin_amdgcn_readlane(metaW, 2);
      // Control workgroup: the two images of tree tnn (one per number of draws the NEXT decide step can consume).  They depend on
      // which image of tree tn survives this launch; image 0 (the pending move of tree t-1 is rejected, or draws nothing) is by
      // far the likeliest, so a first attempt assumes it and runs while wave 0 is still deciding; once the proposal of tree tn is
      // settled the attempt either stands or is repeated from what really happened.
      const int valid0 = __builtin_amdgcn_readlane(pa0W, 8);
      bool have = false; int haveHyp = 0, havePerr = 0, bigNext = 0;
      Proposal prN; prN.hwm = 0;
      const int hwmP = g.i32(40 + TI_HWM);
      // a tree tnn beyond the wave-register path is never proposed for here: its wave arrays hold 64 node slots, and the walk of a
      // truncated tree need not end (fuzz seed 280: a launch that never returned).  The proposal of tree tn then raises needBig
      // (its size test includes tree tnn), and the tail of this launch takes the next step over.
      const bool drawsNow = drawsAhead && step_fits_wave(hwmNN + 2, 0, nc);
      if (drawsNow) {
        caN.nl = g.i32(40 + TI_NL); caN.ni = g.i32(40 + TI_NI); caN.g = g.i32(40 + TI_G); caN.gn = g.i32(40 + TI_GN); caN.valid = g.i32(40 + TI_VALID);
        caN.logPi = g.f64(1);
        if (!caN.valid) tv_rebuild_cache(curN, m, caN);
      }
      for (int attempt = (drawsNow && spec && valid0) ? 0 : 1; attempt < 2; ++attempt) {
        int paType = __builtin_amdgcn_readlane(pa0W, 0), paStatus = __builtin_amdgcn_readlane(pa0W, 1), paNbA = __builtin_amdgcn_readlane(pa0W, 5);
        if (attempt == 1) {
          // ---------------------------------------------------------- this wave's image of tree tn: tables, verdict
          if (valid) {
            if (lane < prC.hwm) {   // statistics half of the pass: this image's table set (a losing image's set is simply not selected)
              NodeS s; s.mu = iMu.mine(); s.binA = (int16_t)iBinA; s.binB = (int16_t)iBinB; s.insub = (int16_t)iInsub; s.pad = 0;
              NodeP p; p.var = (int16_t)iVar; p.cut = (uint16_t)iCut; p.left = (int16_t)iLeft; p.right = (int16_t)iRight;
              L.S3[slot * nc + lane] = s; L.SP3[slot * nc + lane] = p;
            }
            spin_until(&S.verdict, 1, a.errFlag);
            if (__hip_atomic_load(&S.verdict, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == 1 + candIdx) {
              int needNext = prC.hwm > hwmN ? prC.hwm : hwmN;
              if (t + 1 < a.T && hwmNN + 2 > needNext) needNext = hwmNN + 2;
              const int big = step_fits_wave(needNext, prC.nbA + prC.nbB, nc) ? 0 : 1;
              if (lane == 0) { F.root = prC.node; F.nb = prC.nbA + prC.nbB; F.hwmS = prC.hwm; F.needBig = big; F.sset = slot;
                               F.paType = prC.type; F.paStatus = prC.status; F.paNbA = prC.nbA; }
              if (ctl && perrC != 0 && lane == 0) *a.errFlag |= S4B_ERR_NODE_CAPACITY;
              if (lane == 0) __hip_atomic_store(&F.paGo, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
          }
          if (wv == 1 && lane == 0) S4B_STEP_T(22);
          if (!drawsNow) break;
          spin_until(&F.paGo, 1, a.errFlag);
          if (wv == 1 && lane == 0) S4B_CTL_T(24);
          const int wslot = __builtin_amdgcn_readfirstlane(F.sset);
          bigNext = __builtin_amdgcn_readfirstlane(F.needBig);
          if (bigNext) { have = false; break; }          // the tail of this launch takes the next step over
          if (have && wslot == 1) break;                 // the assumption held
          have = false;
          paType = __builtin_amdgcn_readfirstlane(F.paType); paStatus = __builtin_amdgcn_readfirstlane(F.paStatus); paNbA = __builtin_amdgcn_readfirstlane(F.paNbA);
#pragma unroll
          for (int j = 0; j < MTJ; ++j) { const int i = lane + j * 64; if (i < MTW) ((uint32_t*)&F.rngB[candIdx])[i] = ((const uint32_t*)&S.rng[wslot])[i]; }
        }
        // the decide step of the next launch consumes one uniform for the accept test plus two per leaf of the tree it ends with
        const int drawsAccept = paStatus == 1 ? 1 : 0;
        const int nlNow = paNbA;
        const int nlAcc = paType == MOVE_BIRTH ? nlNow + 1 : (paType == MOVE_DEATH ? nlNow - 1 : nlNow);
        const int hyp0 = drawsAccept + 2 * nlNow, hyp1 = drawsAccept + 2 * nlAcc;
        const bool exists = candIdx == 0 || (drawsAccept == 1 && hyp1 != hyp0);
        if (!exists) continue;                            // one image is enough
        const int hyp = candIdx == 0 ? hyp0 : hyp1;
        WaveRng rng; rng.open(&F.rngB[candIdx]);
        rng_advance(&rng, hyp);
        rng.count = 0;
        tbN.prop = curN;
        tbN.binA.r = -1; tbN.binB.r = -1; tbN.insub.r = 0; tbN.list.r = 0;
        if (wv == 1 && lane == 0) S4B_CTL_T(25);
        const int perr = propose(curN, hwmP, m, &rng, &prN, tbN, caN);
        if (wv == 1 && lane == 0) S4B_CTL_T(26);
        rng.close(); F.rngB[candIdx].pad = 0;
        have = true; haveHyp = hyp; havePerr = perr;
      }
      if (drawsAhead) {
        const CandSet cdOut = cand_view(a, (t + 1) & 1, candIdx);
        if (!have) { if (lane == 0) cdOut.meta[0] = 0; }
        else {
          int16_t* const sO = cdOut.slab;
          const int cntOut = prN.hwm;
          wave_tree_store(tbN.prop, sO + SF_VAR * nc, (uint16_t*)(sO + SF_CUT * nc), sO + SF_LEFT * nc, sO + SF_RIGHT * nc, sO + SF_PARENT * nc, cntOut, lane);
          if (lane < cntOut) { sO[SF_BINA * nc + lane] = (int16_t)tbN.binA.r; sO[SF_BINB * nc + lane] = (int16_t)tbN.binB.r; cdOut.insub[lane] = (uint8_t)tbN.insub.r;
                               sO[SF_NA * nc + lane] = (int16_t)tbN.prop.na.r; sO[SF_DEP * nc + lane] = (int16_t)tbN.prop.dep.r; }
          if (laneIn) {   // snapshot of tree tnn: what the launch after the next decides from
            sO[SF_CVAR * nc + lane] = (int16_t)curN.var.r; ((uint16_t*)sO)[SF_CCUT * nc + lane] = (uint16_t)curN.cut.r; sO[SF_CLEFT * nc + lane] = (int16_t)curN.left.r;
            sO[SF_CRIGHT * nc + lane] = (int16_t)curN.right.r; sO[SF_CPARENT * nc + lane] = (int16_t)curN.parent.r; sO[SF_CNA * nc + lane] = (int16_t)curN.na.r;
            sO[SF_CDEP * nc + lane] = (int16_t)curN.dep.r; sO[SF_CLEAF * nc + lane] = (int16_t)caN.leaf.r; sO[SF_CPRE * nc + lane] = (int16_t)caN.pre.r;
            sO[SF_CPOST * nc + lane] = (int16_t)caN.post.r; cdOut.snapMu[lane] = muN.mine(); cdOut.snapCnt[lane] = cntN;
          }
          step_header_store(prN, hwmP, caN.nl, caN.ni, caN.g, caN.gn, caN.logPi, cdOut.head, lane);
#pragma unroll
          for (int j = 0; j < MTJ; ++j) { const int i = lane + j * 64; mtw[j] = ((const uint32_t*)&F.rngB[candIdx])[i < MTW ? i : 0]; }
#pragma unroll
          for (int j = 0; j < MTJ; ++j) { const int i = lane + j * 64; if (i < MTW) ((uint32_t*)cdOut.rng)[i] = mtw[j]; }
          if (lane < 3) cdOut.meta[lane] = lane == 0 ? 1 : (lane == 1 ? haveHyp : havePerr);
          if (wv == 1 && lane == 0) S4B_CTL_T(27);
        }
      }
    }
    if (lane == 0 && wv == 1) S4B_STEP_T(17);
    if (lane == 0 && wv == 2) S4B_STEP_T(18);
    S4B_ARRIVE();
    S4B_CP(2);
    __syncthreads();
    S4B_CP(3);
    if (!ctl) {
#pragma unroll
      for (int j = 0; j < F_PF; ++j) {   // this thread's first quads, requested by loader thread threadIdx.x
        const int sl = j * F_CTL + (int)threadIdx.x;
        P.r01[j] = L.hR01[sl]; P.r23[j] = L.hR23[sl]; P.lf4[j] = L.hLf[sl]; P.pl4[j] = L.hPl[sl];
        if (WEIGHTED) { P.w01[WEIGHTED ? j : 0] = L.hW01[sl]; P.w23[WEIGHTED ? j : 0] = L.hW23[sl]; }
      }
    }
  }

  // ==================================================================== the O(N) pass
  if (threadIdx.x == 3 * 64) S4B_STEP_T(8);
  const int prevAcc = F.prevAcc, prevRoot = F.prevRoot, root = F.root, nb = F.nb;
  StepLds Lp = L;
  Lp.S = L.S3 + F.sset * nc; Lp.SP = L.SP3 + F.sset * nc;
  if (ctl) { /* no observations here */ }
  else if (!doPropose) step_pass<4, true, false, WEIGHTED, true>(a, tn, tt, Lp, root, prevRoot, prevAcc, 0, 0, P, q0, stride, partOut);
  else if (!doDecide) {
    if (nb <= 4) step_pass<4, false, true, WEIGHTED, true>(a, tn, tt, Lp, root, prevRoot, 0, 0, nb, P, q0, stride, partOut);
    else {
      step_pass<8, false, true, WEIGHTED, true>(a, tn, tt, Lp, root, prevRoot, 0, 0, nb, P, q0, stride, partOut);
      for (int base = 8; base < nb; base += 8) { __syncthreads(); step_pass<8, false, true, WEIGHTED, false>(a, tn, tt, Lp, root, prevRoot, 0, base, nb, P, q0, stride, partOut); }
    }
  } else if (nb <= 4) step_pass<4, true, true, WEIGHTED, true>(a, tn, tt, Lp, root, prevRoot, prevAcc, 0, nb, P, q0, stride, partOut);
  else if (nb <= 8 || WEIGHTED) {
    step_pass<8, true, true, WEIGHTED, true>(a, tn, tt, Lp, root, prevRoot, prevAcc, 0, nb, P, q0, stride, partOut);
    for (int base = 8; base < nb; base += 8) { __syncthreads(); step_pass<8, false, true, WEIGHTED, false>(a, tn, tt, Lp, root, prevRoot, prevAcc, base, nb, P, q0, stride, partOut); }
  } else {
    step_pass<NBMAX, true, true, WEIGHTED, true>(a, tn, tt, Lp, root, prevRoot, prevAcc, 0, nb, P, q0, stride, partOut);
    // further bin passes read the residual this thread has just written
    for (int base = NBMAX; base < nb; base += NBMAX) { __syncthreads(); step_pass<NBMAX, false, true, WEIGHTED, false>(a, tn, tt, Lp, root, prevRoot, prevAcc, base, nb, P, q0, stride, partOut); }
  }

#ifdef S4B_LIGHT_TIMING
  if (doDecide && doPropose && (int)blockIdx.x == 100 && lane == 0) {
    atomicAdd(&g_arr[wv], (unsigned long long)(tArr - tL0));
    if (wv == 3) { atomicAdd(&g_arr[8], (unsigned long long)(wall_clock64() - tL0)); atomicAdd(&g_arr[9], 1ull); }
  }
#endif
#ifdef S4B_CONTROL_TIMING
  if (threadIdx.x == 3 * 64) S4B_STEP_T(9);
  if (threadIdx.x == 0 && doDecide && doPropose) atomicAdd(&g_wgE[blockIdx.x], (unsigned long long)wall_clock64());
#endif
  // ==================================================================== tail: the next control step does not fit the wave path
  S4B_CP(4);
  if (!(doPropose && F.needBig)) return;
  __syncthreads();
  S4B_CP(5);
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int k = __hip_atomic_fetch_add(a.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    F.last = (k == (int)gridDim.x - 1) ? 1 : 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  __syncthreads();
  if (!F.last) return;
#ifdef S4B_TUNING
#define S4B_DBG_MARK(bit) do { if (threadIdx.x == 0) __hip_atomic_store(&g_dbgMark, (t << 8) | (bit), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); } while (0)
#else
#define S4B_DBG_MARK(bit)
#endif
  S4B_DBG_MARK(16);
  {
    // totals of every bin of statistics(tn) to global memory, fixed order
    const int nbAll = F.nb, grid = a.gridF;
    for (int k = wv; k < nbAll; k += FBLOCK / 64) {
      double sm = 0.0, c = 0.0, wt = 0.0;
      for (int b = lane; b < grid; b += 64) { sm += partOut[(size_t)k * grid + b]; c += partOut[kindStride + (size_t)k * grid + b]; if (WEIGHTED) wt += partOut[2 * kindStride + (size_t)k * grid + b]; }
      sm = wave_sum(sm); c = wave_sum(c); wt = wave_sum(wt);
      if (lane == 0) { a.binSum[k] = sm; a.binCnt[k] = c; if (WEIGHTED) a.binWt[k] = wt; }
    }
    // generator: the state this launch left in slot (t+1)&1 continues in slot t&1, where launch t+2 expects it
    MTState* rngNext = a.rngF + (t & 1);
    const MTState* rngCur = a.rngF + ((t + 1) & 1);
    for (int i = threadIdx.x; i < (int)(sizeof(MTState) / 4); i += FBLOCK) ((uint32_t*)rngNext)[i] = ((const uint32_t*)rngCur)[i];
    cache_to_main(a, tn);
    __threadfence();
    __syncthreads();
    const int next = t + 1 < a.T ? t + 1 : -1;
    S4B_DBG_MARK(17);
    if (threadIdx.x == 0) { BartArrays b = a; b.rng = rngNext; b.rng->pad = 0; control_global_path(b, tn, next, S.scratch[0]); }
    S4B_DBG_MARK(18);
    __threadfence();
    __syncthreads();
    if (next >= 0) snapshot_from_main(a, next);
    S4B_DBG_MARK(19);
    if (threadIdx.x == 0) { a.preDone[(t + 1) & 1] = 1; *a.ticket = 0; }
  }
}

}  // namespace s4b
