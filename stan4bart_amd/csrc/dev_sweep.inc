// k_sweep: the PERSISTENT tree sweep — ONE launch per sweep (the device-only helpers and the kernel bodies of the translation unit
// dev_sweep.hip, which includes this file once, after the shared headers and dev_sweep_api.hpp).
//
// k_step pays, per tree, one kernel boundary (1.7 us), a cold first touch of everything another XCD wrote (3 us: partials, scratch
// set, proposal images, generator) and 22 B per observation of residual / leaf-plane traffic, and its O(N) pass (4.5 us) starts only
// when the decision is out.  Here gridDim.x - 1 PASS workgroups and one CONTROL workgroup stay resident for the whole sweep
// (reference semantics: one sweep = T sequential tree updates, src/init.cpp:824, SURVEY 3.4), and the 8 waves of a workgroup have
// fixed ROLES that never meet at a workgroup barrier — they hand over through counters in LDS:
//   wave 0       DECIDER: totals of statistics(t-1) -> decide(t-1) (accept / reject, leaf draws) -> apply tables.  Redundantly in
//                every workgroup (k_step's trick, kept), from the workgroup's OWN on-chip state: nothing of the control state
//                crosses workgroups, nothing is cold.
//   waves 1, 2   IMAGE waves: as soon as the proposal of tree t is settled they draw the two images of the proposal of tree t+1
//                (one per number of draws decide(t) can consume) into LDS slots — a whole step ahead of their use.
//   wave 3       EXCHANGE: polls the exchange words of statistics(t-1) until every workgroup has arrived, hands the totals to wave 0,
//                re-arms the exchange buffer after next; then computes the leaf values tree t-1 gets IF ITS MOVE IS NOT ACCEPTED (the
//                common outcome: they depend on nothing the accept test produces) beside wave 0's likelihood arithmetic, so that a
//                "no" sends verdict, old and new leaf values out together and the pass waves fold both with one 16-byte table read.
//   waves 4-7    PASS waves (one per SIMD): the residual of their observations (16 per thread) lives in REGISTERS for all T trees.  While wave 0
//                waits for the totals and decides, they ROUTE their observations under both images of tree t (leaf ids of the
//                tree, predictor columns: nothing of that depends on the pending decision); once the decision and the surviving
//                image are known only arithmetic is left: fold tree t-1 in (two table reads per observation), add the partial
//                residual to the bins of the surviving image, one block reduction.  Relabelling under an accepted move needs no
//                routing either: the leaf an observation moves to is the B bin it was counted in one step earlier.
//                Wave 4 also stages tree t+1 from the main arrays for the image waves.
//   * per tree a thread reads 2 B (leaf id) + 2-6 B (predictor columns) per observation and writes 2 B under an accepted move,
//     instead of 22 B;
//   * the only words that cross workgroups are the bin partials: per bin two 64-bit fixed-point words ADDED into 8 copies with
//     agent-scope integer atomics (xc_publish, dev_step_shared.hpp) — order-free, hence deterministic, every workgroup reads the same
//     totals — polled by one wave per workgroup (8 x 2 nb words); profiles/r04_sweep_probe.txt: 2.1 us (4 bins) .. 3.3 us (8 bins)
//     against 4.8 .. 6.5 us for an all-to-all gather of per-workgroup partials and ~5 us for k_step's boundary + cold reduce.
//   * SPECULATION (round 5): the outcome "the move of tree t-1 is not accepted and image 0 of tree t is its proposal" (98 % of the steps
//     of a stationary chain) needs nothing of the accept test: wave 3's leaf values and the routing under image 0 are there 1.2 us after
//     the totals.  The pass waves gather the statistics of tree t with tree t-1 folded in on the fly and PUBLISH them before the verdict,
//     into the first of two exchange rings: the exchange runs beside the accept test, the chain of a step is totals -> leaf values ->
//     statistics -> exchange, and the decider is off it.  A verdict that does not bear the outcome out sends the statistics, gathered
//     the old way, to the second ring, where every workgroup then looks (same verdict everywhere).  See the pass waves and wave 3.
// The control workgroup owns no observations: it decides like the others and writes the decided trees (and the trace) to the main
// arrays, which nobody reads again before the next sweep.
// What does not fit (a tree beyond the 64 node slots of the wave-register control path) ends the launch early in exactly the state
// k_step expects at the next launch (residual, partials, scratch set, generator slot written back, the sequential global-memory
// control step run by the last workgroup); the host finishes that sweep with k_step launches (status word).
namespace s4b {
#ifdef S4B_SWEEP_WG
// per-workgroup stamps of the exchange (`-DS4B_SWEEP_WGT` alone: nothing else is timed, every workgroup carries the same four atomics per step)
#define SW_W(i) do { if (lane == 0 && t > 0 && t < T && (int)SW_BX < 256) atomicAdd(&g_wg[SW_BX * 16 + (i)], (unsigned long long)wall_clock64() - (unsigned long long)F.t0[t & 3]); } while (0)
__device__ unsigned long long g_pubMax[8], g_pubMin[8];     // wall clock of the last / first speculative publish of step t (slot t & 7)
// per workgroup: [0] sum of (speculative publish - totals seen) [1] steps [2] sum of the wall clock when the totals were seen [3] steps
//                [4] sum of (totals of step t+1 seen - last speculative publish of step t) [5] steps [6] sum of (last - first publish) [7] -
//                after the totals were seen, steps that speculate: [8] wave 3's specReady [9] wave 5 starts the statistics [10] wave 4 past the barrier of the reduction [11] wave 5 through with the step
__device__ unsigned long long g_wg[256 * 16];
__device__ unsigned long long g_wd[256 * 64];
void sweep_wg_fetch(unsigned long long* out) {   // (reads and clears)
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wg), sizeof(g_wg));
  static unsigned long long z[256 * 16]; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wg), z, sizeof(z));
}
// (out of line: inlined into the pass waves' loop, the two atomics trip the compiler — "Illegal instruction detected: Operand has incorrect register class" on a null test of the shared-memory aperture)
// ([16 + i]: how often that phase took more than 3 us; [24 + i]: its maximum)
__device__ __attribute__((noinline)) void sw_dur_add(int idx, unsigned long long v) { atomicAdd(&g_wd[idx], v); atomicAdd(&g_wd[idx + 8], 1ull); if (v > 300ull) atomicAdd(&g_wd[idx + 16], 1ull); atomicMax(&g_wd[idx + 24], v); }
// ([32 + i] sums, [48 + i] counts: moments of a step on the clock of "this workgroup saw the totals of the step": 0 decider past the totals, 1 decider has wave 3's leaf
//  values, 2 decider past its wait for the pass waves, 3 verdict out, 4 decider's step ends, 5 wave 1 starts drawing the ahead image, 6 wave 1 has drawn it, 7 proposal settled (paGo))
__device__ __attribute__((noinline)) void sw_abs_add(int idx, long long v) { atomicAdd(&g_wd[idx], (unsigned long long)v); atomicAdd(&g_wd[idx + 16], 1ull); }
#ifdef S4B_SWEEP_WGD
#define SW_ABS(i) do { if (lane == 0 && t > 1 && t + 1 < T && (int)SW_BX < 256) sw_abs_add((int)SW_BX * 64 + 32 + (i), wall_clock64() - F.t0[t & 3]); } while (0)
#endif
void sweep_wd_fetch(unsigned long long* out) {   // (reads and clears)
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wd), sizeof(g_wd));
  static unsigned long long z[256 * 64]; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wd), z, sizeof(z));
}
#endif
#ifndef S4B_SWEEP_WG
#define SW_W(i)
#endif
// (`make wgd`, -DS4B_SWEEP_WGD on top of the stamps of `make wgt`: durations of the pass waves' phases and moments of the decider and of image wave 1 — out-of-line calls
// with global atomics in the control waves: they cost a microsecond per step, the exchange stamps of `make wgt` alone do not)
#ifndef S4B_SWEEP_WGD
#define SW_D(i)
#define SW_D0()
#define SW_DDECL()
#define SW_ABS(i)
#else
#define SW_DDECL() long long tDur = 0
// durations of pass wave 5's phases (linear statistics), g_wd[workgroup][i] sums and [8 + i] counts: [0] end of the previous step -> leaf ids of the next tree requested,
// staging, [1] wait for the image drawn ahead, [2] routing under it, [3] wait for wave 3's leaf values, [4] the ahead pass, [5] wait for the verdict + fold, [6] the step done the old way
#define SW_D0() tDur = wall_clock64()
#define SW_D(i) do { const long long nw_ = wall_clock64(); if (pw == 1 && lane == 0 && t > 1 && t + 1 < T && (int)SW_BX < 256 && tDur != 0) sw_dur_add((int)SW_BX * 64 + (i), (unsigned long long)(nw_ - tDur)); tDur = nw_; } while (0)
#endif
#ifdef S4B_SWEEP_TIMING
#define SW_TIMED_WG (SW_GX == 1 ? 0 : 100)     // (the instrumented workgroup: 100; the only one of a one-workgroup launch)
// phase timers (100 MHz clock) of workgroup 100, accumulated in LDS (F.tacc: no global traffic inside the steps) and flushed to g_sw
// when the launch ends; `make sweeptiming`, printed by s4b_profile_sweep (dev_hip.hip profile_sweep_persistent).  Slots:
//   relative to the moment the wave that takes the stamp finished its previous step (SW_T):
//     [0] steps  [7] sum of bins  [8] steps routed after the decision  [35] steps whose leaf values went out with the verdict
//     [1] wave 3: totals gathered  [2] wave 4: images there  [3] both images routed  [4] tables + proposal there  [5] arithmetic done  [6] published
//     [9] decider: totals seen  [10] verdict  [11] tables out  [12] step end   [16..19] waves 4..7 folded in   [30..33] statistics phase (sweep_stats)
//   absolute timeline, relative to the moment this workgroup saw the totals of the step complete (SW_A; SW_AP: of the previous step):
//     [40] step  [41] decider sees totals  [42] verdict + old values out  [43] new values out  [44] wave 5 routed  [45] past foldReady
//     [46] old values folded  [47] tables + proposal seen  [48] new values folded  [49] statistics reduced  [50] published  [51] wave 3's leaf values
//     [52] proposal settled  [53, 54] foldReady stored -> wave 4 / 5 past their wait
//   late steps (wave 5 still routing when foldReady was stored): [55] count  [56] by how much  [57] routing time  [58] images seen  [59] early-verdict steps
//     among them  [28] wait for the images  [20..23] by move type of image 0  [60, 61] the other steps: routing time, images seen
//   image waves: [24..27] propose() time by move type, [36..39] counts, [62] without a valid move, [63] start of the drawing step -> propose();
//     drawings that took > 8 us: [15] count  [13] generator copied  [14] wait for the staged tree  [29] tree loaded + generator advanced  [34] propose()
//     [70] image stored; all drawings: [64] cache invalid  [65] generator block renewed  [66..68] tree loaded / cache / generator opened  [69] count
__device__ unsigned long long g_sw[128];
void sweep_timing_fetch(unsigned long long* out) {   // (reads and clears)
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sw), sizeof(g_sw));
  unsigned long long z[128] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_sw), z, sizeof(z));
}
void sweep_decide_fetch(unsigned long long* out) {   // (reads and clears)
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dec), sizeof(g_dec));
  unsigned long long z[16] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_dec), z, sizeof(z));
}
#define SW_T(i) do { if ((int)SW_BX == SW_TIMED_WG && lane == 0 && t > 0 && t < T) atomicAdd(&F.tacc[i], (unsigned long long)(wall_clock64() - tStep)); } while (0)
#define SW_MARK() tStep = wall_clock64()
#define SW_AP(i) do { if ((int)SW_BX == SW_TIMED_WG && lane == 0 && t > 1 && t < T) atomicAdd(&F.tacc[i], (unsigned long long)(wall_clock64() - F.t0[(t - 1) & 3])); } while (0)
// absolute timeline of a step: SW_A(i) adds (now - the moment the totals of THIS step were complete in this workgroup), signed
#define SW_A(i) do { if ((int)SW_BX == SW_TIMED_WG && lane == 0 && t > 0 && t < T) atomicAdd(&F.tacc[i], (unsigned long long)(wall_clock64() - F.t0[t & 3])); } while (0)
// (the speculative path: straight to g_sw — [88] steps borne out [89] steps that speculated; timeline like SW_A: [90] wave 5 starts the speculative statistics
//  [91] wave 4 has published them [92] wave 5 past foldReady [93] wave 5 through with the step [94] wave 3 past paGo (its step ends) [95] decider's step ends)
#define SW_G(i) do { if ((int)SW_BX == SW_TIMED_WG && lane == 0 && t > 0 && t < T) atomicAdd(&g_sw[i], (unsigned long long)(wall_clock64() - F.t0[t & 3])); } while (0)
#else
#define SW_G(i)
#define SW_T(i)
#define SW_MARK()
#define SW_A(i)
#define SW_AP(i)
#endif
constexpr int S4B_PRIO_DEC = 1, S4B_PRIO_IMG = 1, S4B_PRIO_XCH = 3, S4B_PRIO_SPEC = 2;   // wave priorities: decider, image waves, exchange wave, a pass wave in its speculative statistics
constexpr int S4B_POLL_DELAY = 40, S4B_POLL_SLEEP = 2;     // the exchange wave's poll: s_sleep before the first look at the exchange words / between two looks
constexpr long long SW_ROLL_TICKS = 20000;   // 200 us of the 100 MHz wall clock: a launch on a free device has all its workgroups running within a few microseconds

struct SweepModel { double pg[64], lpg[64], l1pg[64], li0[64], li1[64]; int nc0[64], nc1[64]; double sigma; };
struct SweepShared {
  // the decided tree t-1, for the pass (written by wave 0 before tablesReady = t)
  int prevAcc, prevRoot, prevDeath;
  // the settled proposal of tree t (written by the wave that settles it before paGo = t + 1)
  int root, nb, needBig, sset, paType, paStatus, paNbA;
  int selSlot[2];        // image slot (0 / 1) that holds the surviving proposal of the tree with that parity of index
  int paGo, foldReady, tablesReady;
  int rng0Copied, rng1Copied;   // >= k once image wave 1 / 2 no longer reads the generator the surviving proposal of tree k left behind (its image of tree k+1 is final)
  int img0Ready, img1Ready;     // >= k once the FINAL image 0 / 1 of tree k is in its slot (or marked absent)
  int pre0Copied;               // >= k once wave 1 has taken what drawing image 0 of tree k+1 AHEAD needs from image 0 of tree k (or draws nothing ahead)
  int staged;            // k once tree k sits in its stage (trees 0 .. k)
  int bar;               // arrivals at the barriers of the pass waves
  int published;         // t + 1 once this workgroup has added its partials of statistics(t) to the exchange words
  int abort, last;
  int specReady;         // (t << 1) | valid once wave 3 has finished its early leaf values of step t (valid: they are in A[].muNew)
  int specNb[2];         // by parity of t: bins of the statistics published BEFORE the verdict in step t (0: none), written with specReady.  (By parity: with the linear
                         // statistics the exchange wave publishes itself and may be a step ahead of a pass wave that has yet to read the word of its step)
  int publishedAlt;      // like published, for the statistics a step publishes again after a speculation that failed
  int passSeen;          // pass waves x steps they are through with (the decider of step t+1 overwrites what they read in step t)
  int specCnt;           // leaves with observations among them (two uniforms each)
  int bothStep;          // t when foldReady = t came with BOTH halves of the leaf-value table (move not accepted, wave 3's values)
  long long t0[4];       // (instrumented build) moment the totals of step t were complete in this workgroup
  long long tFold;
  unsigned long long tacc[64];   // (instrumented build) phase timers, flushed to g_sw when the launch ends: no global traffic inside the steps
  int decDone;           // t once wave 0 has written / checked the leaf-value table of step t (wave 3 of step t + 1 writes it next)
  // linear statistics
  int linReady;          // t once F.specNb of step t is written (linear statistics: the pass waves wait for THIS word — it follows wave 3's wait for the ahead pass of the step
                         // before; specReady, which the decider waits for, goes out before that wait)
  int pre0Ready;         // >= k once image 0 of tree k drawn AHEAD (wave 1, two steps before the tree is decided) is in its slot, or is known not to be drawn
  int aheadId[3];        // by image slot: the drawing number of that ahead image (0: none) — written before pre0Ready
  int aheadNb[3];        // ... and its bin count.  (The pass waves decide from THESE words whether to run the ahead pass: the image itself may be drawn again while a
                         // late wave still looks at it, and four waves that read a half-written header need not agree — they meet at a barrier inside the pass)
  int statArr;           // pass waves through with the statistics in flight (the fourth to arrive publishes)
  int preArrA, preArrB;
  int preDoneA, preDoneB;// k once the pass waves are through with the ahead pass for tree k of the step before (A: beside its verdict; B: after a step redone the old way)
  int preNb[2], preSeq[2];   // by parity of k: bins of the ahead statistics of tree k that sit in the pre-sum tables (0: none), drawing number of the image they were gathered under
  double totS[64], totC[64];
  MTState rngB[2];
};
struct SweepLds { NodeS* S; NodeP* SP; NodeA* A; uint8_t* Ain; uint8_t* b2n; double* redS; int* redN; unsigned char* img; TreeStage* stage;
                  NodeS* SA; NodeP* AP;      // SA / AP: apply-half routing tables of the streaming variant (the decided tree t-1 as proposed: node -> itself, rules)
                  unsigned* ctab; double* preS; int* preC; NodeA* zeroA; double* dtab; };     // dtab: old - new leaf value of the tree before, by parity of the step (the ahead pass folds through it)   // linear statistics: contingency counts and pre-sums by parity of the tree, a leaf-value table of zeros
__device__ __forceinline__ SweepLds carve_sweep(unsigned char* base) {
  SweepLds L;
  L.S = (NodeS*)base; base += (size_t)SW_SETS * SW_NC * 16;
  L.A = (NodeA*)base; base += (size_t)2 * SW_NC * 16;     // (two tables, by the parity of the step: see sw_apar)
  L.SP = (NodeP*)base; base += (size_t)SW_SETS * SW_NC * 8;
  L.redS = (double*)base; base += (size_t)8 * SW_RED_ROW * 8;
  L.redN = (int*)base; base += (size_t)8 * SW_RED_ROW * 4;
  L.Ain = (uint8_t*)base; base += 64;
  L.b2n = (uint8_t*)base; base += 64;
  L.img = base; base += SW_SLOTS * cand_bytes(SW_NC);
  L.stage = (TreeStage*)base; base += SW_STAGES * stage_bytes();
  L.SA = (NodeS*)base; base += (size_t)SW_NC * 16;
  L.AP = (NodeP*)base; base += (size_t)SW_NC * 8;
  L.zeroA = (NodeA*)base; base += (size_t)SW_NC * 16;
  L.ctab = (unsigned*)base; base += (size_t)2 * SW_CT_WORDS * 4;
  L.preS = (double*)base; base += (size_t)2 * SW_PW * 8 * 8;      // [parity][pass wave][bin]
  L.preC = (int*)base; base += (size_t)2 * 8 * 4;
  L.dtab = (double*)base;
  return L;
}
__device__ __forceinline__ int sw_slot(int tree, int c) { return c == 0 ? tree % 3 : 3 + (tree & 1); }
__device__ __forceinline__ CandSet cand_lds(unsigned char* img, int tree, int c) {     // image c of tree `tree`
  unsigned char* base = img + (size_t)sw_slot(tree, c) * cand_bytes(SW_NC);
  constexpr int nc = SW_NC;
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
// was the speculation of step t ("the move of tree t-1 is not accepted, image 0 of tree t is its proposal, nbSpec bins") borne out?  Read after
// paGo(t+1); the decider does not touch these words again before every pass wave is through with the step (passSeen).
template <class Shared>
__device__ __forceinline__ bool sweep_spec_confirmed(const Shared& F, int t, int nbSpec) {
  return __builtin_amdgcn_readfirstlane(F.bothStep) == t && __builtin_amdgcn_readfirstlane(F.sset) == 1 + sw_slot(t, 0) &&
         __builtin_amdgcn_readfirstlane(F.nb) == nbSpec && __builtin_amdgcn_readfirstlane(F.needBig) == 0;
}
// wait until a monotonic LDS counter reaches `target`; false (and the abort flag up) when it never does — a logic error or a
// workgroup that is not resident: never hang the device
// (the abort flag carries the source line of the wait that gave up first: reported to the host beside the status word)
template <int SLEEP>
__device__ __forceinline__ bool spin_counter_at(int* flag, int target, int* abortFlag, int line) {
  int guard = 0;
  while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < target) {
    __builtin_amdgcn_s_sleep(SLEEP);
    if (++guard > (1 << 21)) { int none = 0; __hip_atomic_compare_exchange_strong(abortFlag, &none, line, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); return false; }
    if (((guard & 1023) == 0) && __hip_atomic_load(abortFlag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return false;
  }
  return true;
}
// (SW_SLEEP: a constant of the kernel body the macro is used in — the streaming variant's waits are long and share their SIMDs with the pass waves' only wave)
#define spin_counter(flag, target, abortFlag) spin_counter_at<SW_SLEEP>(flag, target, abortFlag, __LINE__)
__device__ __forceinline__ unsigned long long xc_load(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// A 0 / ~0 mask the optimiser cannot see through.  Table reads whose results are merged with such masks stay UNCONDITIONAL: written
// as selects, the compiler sinks the reads into per-observation branches (one s_waitcnt per read: the 64 table reads of a thread's
// 16 observations then cost 64 LDS round trips in a row instead of two).
__device__ __forceinline__ unsigned sw_mask(bool c) { unsigned m = c ? 0xffffffffu : 0u; asm("" : "+v"(m)); return m; }
__device__ __forceinline__ unsigned sw_sel(unsigned m, unsigned a, unsigned b) { return b ^ ((a ^ b) & m); }   // m ? a : b
// one wave: tree tr, main arrays -> stage[tr & 1]
__device__ __forceinline__ void stage_tree(const BartArrays& a, TreeStage* stage, int tr, int l) {
  TreeStage* st = stage + (tr % SW_STAGES);
  const int nc = a.nc;
  const size_t o = (size_t)tr * nc, ts = (size_t)a.T * nc, tT = (size_t)a.T;
  const bool in = l < nc;
  const unsigned li = in ? (unsigned)l : 0u;
  // (all requests first, unconditional — li is a valid index either way —, then the stores)
  int16_t rowv[TF_COUNT];
#pragma unroll
  for (int r = 0; r < TF_COUNT; ++r) rowv[r] = (a.treeI16 + (size_t)r * ts + o)[li];
  const double muv = a.mu[o + li]; const int cntv = a.cnt[o + li];
  const int scv = a.treeI32[(size_t)(l < TI_COUNT ? l : 0) * tT + tr];
  const double lpv = a.clogpi[tr];
  const unsigned inM = sw_mask(in);
#pragma unroll
  for (int r = 0; r < TF_COUNT; ++r) {
    const unsigned dflt = (unsigned)(int)(int16_t)(r == TF_VAR ? NODE_FREE : (r == TF_CUT ? 0 : -1));
    st->row[r][l] = (int16_t)sw_sel(inM, (unsigned)(int)rowv[r], dflt);
  }
  st->mu[l] = in ? muv : 0.0; st->cnt[l] = in ? cntv : 0;
  if (l < TI_COUNT) st->sc[l] = scv;
  if (l == 0) st->logPi = lpv;
}
// barrier of the pass waves (the other waves of the workgroup never take part): one arrival per wave on an LDS counter
struct PassBar { int* ctr; int* abortFlag; int epoch; unsigned long long* tacc; double* totS; double* totC; bool solo; int* arr; };   // totS / totC: solo mode (the reduction's result is the total; a flag, not a
                                                                                                                               // null pointer: a pointer that is an LDS address or null trips the compiler)
__device__ __forceinline__ void pass_barrier(PassBar& b) {
  b.epoch += SW_PW;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(b.ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  int guard = 0;
  while (__hip_atomic_load(b.ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < b.epoch) {
    if (++guard > (1 << 22)) { __hip_atomic_store(b.abortFlag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); break; }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// The kernel arguments (a ~900-byte struct of pointers) through a pointer the optimiser cannot see through, re-made wherever a
// block of a step needs them: otherwise every field the loop touches is loaded once before the loop and stays live across it —
// hundreds of scalar registers spilled into vector registers, and those into scratch memory.
#define SW_KERNARGS()                                                                                                        \
  auto kp_ = (const __attribute__((address_space(4))) unsigned char*)__builtin_amdgcn_kernarg_segment_ptr(); SW_SLOT_OF(kp_);  \
  asm volatile("" : "+s"(kp_));                                                                                              \
  const BartArrays& a = *(const BartArrays*)kp_;                                                                             \
  const SweepArgs& x = *(const SweepArgs*)(kp_ + (sizeof(BartArrays) + 7) / 8 * 8); (void)x; (void)a
#include "sweep_batch.inc"
// per-observation state of a pass thread: 4 quads.  Packed fields hold one byte per observation of the quad.
// (round 6: the leaf ids too — three trees are in flight per thread since the statistics run a step ahead; node ids of the wave path are < 64)
typedef unsigned lfq_t;
__device__ __forceinline__ lfq_t lfq_pack(us4_t v) { return ((unsigned)v.x & 0xffu) | (((unsigned)v.y & 0xffu) << 8) | (((unsigned)v.z & 0xffu) << 16) | ((unsigned)v.w << 24); }
#define LFQ4(w) {(w) & 63u, ((w) >> 8) & 63u, ((w) >> 16) & 63u, ((w) >> 24) & 63u}
struct SweepObs {
  double r[SW_PF][4];        // the residual (all trees folded in except the ones still in flight)
  lfq_t lfPrev[SW_PF];      // node id of the observation's leaf in the previous tree (before its pending move), one byte per observation of the quad
  unsigned bbPrev[SW_PF];    // its B bin under that tree's surviving proposal (0xff: not under the proposal's node)
};
// B bins of this thread's observations under NI proposals at once (table sets S[i] / SP[i], node root[i]; have[i]: the proposal
// exists): level-synchronous — the loads of one level of all 16 observations under all proposals are in flight together.
// 0xff: the observation is not under the proposal's node.
template <int NI>
__device__ __forceinline__ void sweep_route(const BartArrays& a, const NodeS* const (&S)[NI], const NodeP* const (&SP)[NI], const int (&root)[NI], const bool (&have)[NI],
                                            const lfq_t (&lf)[SW_PF], int64_t q0, int64_t stride, int64_t nQuads, unsigned (&bb)[NI][SW_PF]) {
  NodeP pr[NI]; int rootVar[NI];
  us4_t xq[NI][SW_PF];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    pr[i] = SP[i][have[i] ? (root[i] & (SW_NC - 1)) : 0];
    rootVar[i] = have[i] ? (int)pr[i].var : -1;    // < 0: no subtree under the node (a death, or no proposal): nothing is counted twice
    const uint16_t* __restrict__ col = a.xbin + (size_t)((rootVar[i] >= 0 && rootVar[i] < a.P) ? rootVar[i] : 0) * a.npad;     // (a predictor index out of a half-written table must not leave the matrix)
#pragma unroll
    for (int j = 0; j < SW_PF; ++j) {
      const int64_t qd = q0 + (int64_t)j * stride;
      xq[i][j].x = 0; xq[i][j].y = 0; xq[i][j].z = 0; xq[i][j].w = 0; bb[i][j] = 0xffffffffu;
      if (rootVar[i] >= 0 && qd < nQuads) xq[i][j] = *reinterpret_cast<const us4_t*>(col + (qd << 2));
    }
  }
  // (every phase below first issues ALL its table reads / loads into arrays and only then uses them: interleaved with their uses
  // the compiler keeps source order — one LDS round trip per read)
  int cur[NI][SW_PF][4];
  unsigned anyM = 0u;
  unsigned insv[NI][SW_PF][4];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
#pragma unroll
    for (int j = 0; j < SW_PF; ++j) {
      const unsigned l4[4] = LFQ4(lf[j]);
#pragma unroll
      for (int e = 0; e < 4; ++e) insv[i][j][e] = (unsigned)(int)S[i][l4[e]].insub;        // (leaf ids beyond n are 0, a valid index)
    }
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int cL = rootVar[i] >= 0 ? ((int)pr[i].left & (SW_NC - 1)) : 0, cR = rootVar[i] >= 0 ? ((int)pr[i].right & (SW_NC - 1)) : 0;
    const unsigned leafLM = sw_mask((int)SP[i][cL].var < 0), leafRM = sw_mask((int)SP[i][cR].var < 0);
    const unsigned bL = (unsigned)(int)S[i][cL].binB & 0xffu, bR = (unsigned)(int)S[i][cR].binB & 0xffu;
    const unsigned rootM = sw_mask(rootVar[i] >= 0);
#pragma unroll
    for (int j = 0; j < SW_PF; ++j) {
      const int64_t qd = q0 + (int64_t)j * stride;
      const int valid = qd < nQuads ? ((a.n - (qd << 2)) >= 4 ? 4 : (int)(a.n - (qd << 2))) : 0;
      const unsigned x4[4] = {xq[i][j].x, xq[i][j].y, xq[i][j].z, xq[i][j].w};
      unsigned packed = 0u;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned insM = (0u - (unsigned)(insv[i][j][e] != 0u)) & rootM & (0u - (unsigned)(e < valid));
        const unsigned goLM = 0u - (unsigned)(x4[e] <= (unsigned)pr[i].cut);
        const unsigned childLeafM = sw_sel(goLM, leafLM, leafRM);
        const unsigned child = sw_sel(goLM, (unsigned)cL, (unsigned)cR);
        const unsigned deeperM = insM & ~childLeafM;
        cur[i][j][e] = (int)sw_sel(deeperM, child, 0xffffffffu);
        const unsigned b = sw_sel(insM & childLeafM, sw_sel(goLM, bL, bR), 0xffu);
        packed |= b << (8 * e);
        anyM |= deeperM;
      }
      bb[i][j] = packed;
    }
  }
  if (anyM == 0u) return;
  // deeper levels (a child of the proposal's node is an internal node: change / swap moves high in the tree), one proposal at a time
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    unsigned actAny = 0u;
#pragma unroll
    for (int j = 0; j < SW_PF; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) actAny |= 0u - (unsigned)(cur[i][j][e] >= 0);
    }
    // (bounded: an image drawn AHEAD may be drawn again while a late pass wave still routes under it — the result is thrown away then, but a walk over
    // half-written tables must end)
    int levels = 0;
    while (actAny != 0u && ++levels <= 2 * S4B_MAX_DEPTH) {
      unsigned xv[SW_PF][4]; unsigned pvc[SW_PF][4], plr[SW_PF][4];     // node record as two words: var | cut << 16, left | right << 16
#pragma unroll
      for (int j = 0; j < SW_PF; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = cur[i][j][e] >= 0 ? (cur[i][j][e] & (SW_NC - 1)) : 0;
          const uint2 w = *reinterpret_cast<const uint2*>(&SP[i][c]);
          pvc[j][e] = w.x; plr[j][e] = w.y;
        }
      }
#pragma unroll
      for (int j = 0; j < SW_PF; ++j) {
        const int64_t i0 = (q0 + (int64_t)j * stride) << 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          // unconditional loads (an inactive cursor reads column 0 at its own observation: valid and cached), all in flight together
          const int64_t ie = (i0 + e) < a.npad ? (i0 + e) : 0;
          const int v = (int)(int16_t)(pvc[j][e] & 0xffffu);
          xv[j][e] = a.xbin[(size_t)((v >= 0 && v < a.P) ? v : 0) * a.npad + (size_t)ie];
        }
      }
      int nd[SW_PF][4]; unsigned ndVar[SW_PF][4], ndBin[SW_PF][4];
#pragma unroll
      for (int j = 0; j < SW_PF; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int raw = (xv[j][e] <= (pvc[j][e] >> 16)) ? (int)(int16_t)(plr[j][e] & 0xffffu) : (int)(int16_t)(plr[j][e] >> 16);
          nd[j][e] = raw >= 0 ? (raw & (SW_NC - 1)) : 0;
        }
      }
#pragma unroll
      for (int j = 0; j < SW_PF; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { ndVar[j][e] = (unsigned)(int)SP[i][nd[j][e]].var; ndBin[j][e] = (unsigned)(int)S[i][nd[j][e]].binB & 0xffu; }
      }
      actAny = 0u;
#pragma unroll
      for (int j = 0; j < SW_PF; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const unsigned actM = 0u - (unsigned)(cur[i][j][e] >= 0);
          const unsigned innerM = 0u - (unsigned)((int)ndVar[j][e] >= 0);
          cur[i][j][e] = (int)sw_sel(actM & innerM, (unsigned)nd[j][e], 0xffffffffu);
          const unsigned oldb = (bb[i][j] >> (8 * e)) & 0xffu;
          const unsigned newb = sw_sel(actM & ~innerM, ndBin[j][e], oldb);
          bb[i][j] = (bb[i][j] & ~(0xffu << (8 * e))) | (newb << (8 * e));
          actAny |= actM & innerM;
        }
      }
    }
  }
}
// statistics of one bin pass: per-thread sums of the partial residual rs over the NB bins [base, base + NB) — A bin (current leaf)
// and B bin (leaf the proposal creates) of every observation —, reduction over the pass waves in a fixed order, and the
// workgroup's contribution to the exchange words.  NB is the EXACT number of bins (the cost of the accumulation is observations x
// bins x 4 instructions: per observation a two-bit one-hot word, per bin a bit extract, the 0.0 / 1.0 factor, one fused
// multiply-add — exact: the product is rs or 0 — and one integer add for the count).
__device__ __forceinline__ int sweep_fresh_lane() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}
// (SKIP: the workgroup's threads own fewer than SW_PF quads each — jMax, uniform —: a launch over few observations leaves the unrolled work of the
// others out; the kernel k_sweep_few: in k_sweep itself the uniform branches cost 1 - 1.8 %)
// (LIN — the AHEAD pass of the linear statistics: the sums stay in the workgroup (preS / preC) and every observation also counts into the contingency
// table ctab[its leaf in the tree BEFORE (keyLf)][each of its bins][copy] with LDS atomics that return nothing — integers: order-free)
// (WT — observation weights, k_sweep_w: wq = this thread's sixteen weights in LDS (quad j at wq + j * SW_PT * 4; 0 beyond n), the sums become sums of
// w (r + mu), and a third statistic per bin, the sum of the weights, travels as bin nbAll + k of the same exchange — sum in the sum field, count 0 —: the
// step then exchanges 2 nbAll "bins", which is why such a launch takes trees of at most 32 bins.  Both are published times wScale, a power of two that brings
// the largest weight into (0.5, 1]: the fixed-point words hold sums of O(1) terms; the gathering side multiplies by its inverse.  The scaling is exact
// both ways; the rounding of each partial to the 2^-55 quantum is not, and is a relative error of up to 2^-55 * max / min weight of a bin's sums: the host
// keeps samplers whose weights span more than 2^30 off this kernel — dev_hip.hip, wRangeOk.)
template <int NB, bool SKIP, bool LIN, bool WT = false, bool BATCH = false>
__device__ __forceinline__ bool sweep_stats(const BartArrays& a, const SweepLds& L, PassBar& bar, const double (&r)[SW_PF][4], const lfq_t (&lf)[SW_PF], const NodeS* __restrict__ Ssel,
                                            const unsigned (&bb)[SW_PF], int64_t q0, int64_t stride, int64_t nQuads, int base, unsigned long long* xcur, double* part_,
                                            bool alsoPart, int pw, int lane, long long tRef = 0,
                                            const lfq_t (*foldLf)[SW_PF] = nullptr, const NodeA* __restrict__ foldA = nullptr, int jMax = SW_PF,
                                            const lfq_t (*keyLf)[SW_PF] = nullptr, unsigned* ctab = nullptr, double* preS = nullptr, const double* __restrict__ foldD = nullptr,
                                            const double* __restrict__ wq = nullptr, int nbAll = 0, double wScale = 1.0) {
  static_assert(!WT || !LIN, "the weighted statistics exist in the default build only, not in the ahead pass of the linear one");
#ifdef S4B_SWEEP_TIMING
#define SWS_T(i, cond) do { if ((int)SW_BX == SW_TIMED_WG && lane == 0 && tRef != 0 && (cond)) atomicAdd(&bar.tacc[i], (unsigned long long)(wall_clock64() - tRef)); } while (0)
#else
#define SWS_T(i, cond)
#endif
  static_assert(NB <= 8, "eight bins per pass");
  double accS[NB]; int accN[NB]; double accW[WT ? NB : 1];
#pragma unroll
  for (int k = 0; k < NB; ++k) { accS[k] = 0.0; accN[k] = 0; if (WT) accW[WT ? k : 0] = 0.0; }
#pragma unroll
  for (int j = 0; j < SW_PF; ++j) {
    if (SKIP && j >= jMax) continue;
    const int64_t qd = q0 + (int64_t)j * stride;
    const int valid = qd < nQuads ? ((a.n - (qd << 2)) >= 4 ? 4 : (int)(a.n - (qd << 2))) : 0;
    double ww[4] = {1.0, 1.0, 1.0, 1.0};
    if constexpr (WT) {
      const double2 w01 = *reinterpret_cast<const double2*>(wq + (size_t)j * SW_PT * 4), w23 = *reinterpret_cast<const double2*>(wq + (size_t)j * SW_PT * 4 + 2);
      ww[0] = w01.x; ww[1] = w01.y; ww[2] = w23.x; ww[3] = w23.y;
    }
    // the observation's leaf in the tree: its value (partial residual = residual + own fit) and its A bin; one quad's reads in flight
    const unsigned l4[4] = LFQ4(lf[j]);
    NodeS ns[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) ns[e] = Ssel[l4[e]];            // (unconditional: leaf ids beyond n are 0)
    NodeA na[4];
    double nd[4] = {0.0, 0.0, 0.0, 0.0};
    if (LIN) {      // (the ahead pass folds the tree before through ONE table of differences old - new value: 8 bytes per observation; its sums are used by nobody else)
      const unsigned pl[4] = LFQ4((*foldLf)[j]);
#pragma unroll
      for (int e = 0; e < 4; ++e) nd[e] = foldD[pl[e] & 63u];
    } else if (foldLf) {
      const unsigned pl[4] = LFQ4((*foldLf)[j]);
#pragma unroll
      for (int e = 0; e < 4; ++e) na[e] = foldA[pl[e] & 63u];
    }
    unsigned kl[4] = {0u, 0u, 0u, 0u};
    if (LIN) { const unsigned k4[4] = LFQ4((*keyLf)[j]); kl[0] = k4[0]; kl[1] = k4[1]; kl[2] = k4[2]; kl[3] = k4[3]; }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned okM = 0u - (unsigned)(e < valid);
      const unsigned sa = ((unsigned)(int)ns[e].binA & 0xffu) - (unsigned)base, sb = ((bb[j] >> (8 * e)) & 0xffu) - (unsigned)base;
      const unsigned bits = ((sa < (unsigned)NB ? 1u << sa : 0u) | (sb < (unsigned)NB ? 1u << sb : 0u)) & okM;
      if (LIN) {
        // (two atomics per observation, unconditional: an observation that is in no bin counts into the dummy row)
        const unsigned cc = (unsigned)lane & (unsigned)(SW_CC - 1), dummy = (unsigned)(SW_NC * 8 * SW_CC) + cc;
        const unsigned row = (kl[e] & 63u) * (unsigned)(8 * SW_CC) + cc;
        const unsigned mA = (0u - (unsigned)(sa < (unsigned)NB)) & okM, mB = (0u - (unsigned)(sb < (unsigned)NB)) & okM;
        const unsigned aA = sw_sel(mA, row + (sa & 7u) * (unsigned)SW_CC, dummy), aB = sw_sel(mB, row + (sb & 7u) * (unsigned)SW_CC, dummy);
        (void)__hip_atomic_fetch_add(ctab + aA, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        (void)__hip_atomic_fetch_add(ctab + aB, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      double rv = r[j][e];
      if (LIN) rv += nd[e];
      else if (foldLf) { rv += na[e].muOld; rv -= na[e].muNew; }      // (the previous tree folded in on the fly, as the fold after the verdict does it: the same bits)
      const double rs0 = e < valid ? rv + ns[e].mu : 0.0;     // (0 x NaN would be NaN: an unused slot must hold a finite value)
      const double rs = WT ? rs0 * ww[e] : rs0;
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        const unsigned mk = (bits >> k) & 1u;
        const double md = __hiloint2double((int)(mk * 0x3ff00000u), 0);
        accS[k] = fma(md, rs, accS[k]);
        if (WT) accW[WT ? k : 0] = fma(md, ww[e], accW[WT ? k : 0]);
        if (!LIN) accN[k] += (int)mk;      // (the ahead pass: the contingency counts hold the bin counts too)
      }
    }
  }
  SWS_T(30, pw == 1);
  SWS_T(31, pw == 1);
  if constexpr (LIN) {
    // the ahead pass: every pass wave sums ITS 64 lanes in registers — halving exchanges: NB - 1 + log2(64 / NB) of them, a fixed order — and leaves one pre-sum per
    // bin; wave 3 adds the four waves' in the order of the waves.  No LDS slots, no barrier between the pass waves.
    constexpr int NP2 = NB <= 4 ? 4 : 8;
    double v[NP2];
#pragma unroll
    for (int k = 0; k < NP2; ++k) v[k] = k < NB ? accS[k] : 0.0;
    wave_sum_bins<NP2>(v, lane);
    const int b = wave_bin_of_lane<NP2>(lane);
    if ((lane & (64 / NP2 - 1)) == 0 && b < NB) preS[pw * 8 + b] = v[0];
    return false;
  }
  // Round 6: no block reduction.  Every pass wave sums its 64 lanes in registers (halving exchanges, a fixed order) and leaves one partial per bin; the LAST of the
  // four waves to arrive adds the four partials in the order of the waves and publishes — nobody waits at a barrier, no 256-entry fold by one wave behind it
  // (the statistics sit on the chain of a step: 2.6 us with the barrier, of which 0.7 us barrier and 0.45 us fold).  Returns whether this wave was the last.
  constexpr int NP2 = NB <= 4 ? 4 : 8;
  double v[NP2]; int cn[NP2];
#pragma unroll
  for (int k = 0; k < NP2; ++k) { v[k] = k < NB ? accS[k] : 0.0; cn[k] = k < NB ? accN[k] : 0; }
  wave_sum_bins<NP2>(v, lane); wave_sum_bins<NP2>(cn, lane);
  const int b = wave_bin_of_lane<NP2>(lane);
  if ((lane & (64 / NP2 - 1)) == 0 && b < NB) { L.redS[pw * 8 + b] = v[0]; L.redN[pw * 8 + b] = cn[0]; }
  if constexpr (WT) {
    double vw[NP2];
#pragma unroll
    for (int k = 0; k < NP2; ++k) vw[k] = k < NB ? accW[WT ? k : 0] : 0.0;
    wave_sum_bins<NP2>(vw, lane);
    if ((lane & (64 / NP2 - 1)) == 0 && b < NB) L.redS[32 + pw * 8 + b] = vw[0];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  int old = 0;
  if (lane == 0) old = __hip_atomic_fetch_add(bar.arr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  old = __builtin_amdgcn_readfirstlane(old);
  if (old != SW_PW - 1) return false;
  if (lane == 0) __hip_atomic_store(bar.arr, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  const int k = lane < NB ? lane : 0;
  const double sm = ((L.redS[k] + L.redS[8 + k]) + L.redS[16 + k]) + L.redS[24 + k];
  const int c = ((L.redN[k] + L.redN[8 + k]) + L.redN[16 + k]) + L.redN[24 + k];
  double wsum = 0.0;
  if constexpr (WT) wsum = ((L.redS[32 + k] + L.redS[40 + k]) + L.redS[48 + k]) + L.redS[56 + k];
  if (lane < NB) {
    if (alsoPart) {
      const size_t kind = (size_t)a.binCap * a.gridF;
      part_[(size_t)(base + k) * a.gridF + SW_BX] = sm;
      part_[kind + (size_t)(base + k) * a.gridF + SW_BX] = (double)c;
      if (WT) part_[2 * kind + (size_t)(base + k) * a.gridF + SW_BX] = wsum;
    }
    // (WT: the instantiation may carry more bins than the step has left — NB = 3 for two —: without weights the surplus lands in slots nobody reads; here the slots
    // behind the last bin ARE the sums of the weights)
    if (WT && base + k >= nbAll) { }
    else if (bar.solo) { bar.totS[base + k] = sm; bar.totC[base + k] = (double)c; if (WT) bar.totS[nbAll + base + k] = wsum; }
    else if (WT) { xc_publish(xcur, base + k, sm * wScale, c, a.errFlag); xc_publish(xcur, nbAll + base + k, wsum * wScale, 0, a.errFlag); }
    else xc_publish(xcur, base + k, sm, c, a.errFlag);
  }
  return true;
}
template <int NB, bool SKIP, bool LIN = false, bool WT = false, bool BATCH = false>
__device__ __forceinline__ bool sweep_stats_n(int n, const BartArrays& a, const SweepLds& L, PassBar& bar, const double (&r)[SW_PF][4], const lfq_t (&lf)[SW_PF], const NodeS* __restrict__ Ssel,
                                              const unsigned (&bb)[SW_PF], int64_t q0, int64_t stride, int64_t nQuads, int base, unsigned long long* xcur, double* part,
                                              bool alsoPart, int pw, int lane, long long tRef = 0,
                                              const lfq_t (*foldLf)[SW_PF] = nullptr, const NodeA* __restrict__ foldA = nullptr, int jMax = SW_PF,
                                              const lfq_t (*keyLf)[SW_PF] = nullptr, unsigned* ctab = nullptr, double* preS = nullptr, const double* __restrict__ foldD = nullptr,
                                              const double* __restrict__ wq = nullptr, int nbAll = 0, double wScale = 1.0) {
  // (one instantiation per bin count would be many copies of the unrolled accumulation: with the control code of the other waves the hot
  // code then overflows the instruction cache and EVERY phase of the step runs at half speed — measured; 3, 5 and 8 cover the
  // usual proposals — a tree of 2-3 leaves + a birth, 4-6 leaves + a change — at a third more work than the exact count at most
  // (a 6-bin instantiation, round 5, stationary chain with 5.0 bins per step on average: 18 spilled registers instead of 14, sweep 2.21 instead of 2.165 ms);
  // more than 8 bins take several passes)
  if (n <= 3) return sweep_stats<3, SKIP, LIN, WT, BATCH>(a, L, bar, r, lf, Ssel, bb, q0, stride, nQuads, base, xcur, part, alsoPart, pw, lane, tRef, foldLf, foldA, jMax, keyLf, ctab, preS, foldD, wq, nbAll, wScale);
  else if (n <= 4) return sweep_stats<4, SKIP, LIN, WT, BATCH>(a, L, bar, r, lf, Ssel, bb, q0, stride, nQuads, base, xcur, part, alsoPart, pw, lane, tRef, foldLf, foldA, jMax, keyLf, ctab, preS, foldD, wq, nbAll, wScale);
  else if (n <= 5) return sweep_stats<5, SKIP, LIN, WT, BATCH>(a, L, bar, r, lf, Ssel, bb, q0, stride, nQuads, base, xcur, part, alsoPart, pw, lane, tRef, foldLf, foldA, jMax, keyLf, ctab, preS, foldD, wq, nbAll, wScale);
  // (the last two branches are the same call and stay two: written as one, register allocation and scheduling of k_sweep* come out differently — 270 000 lines of its assembly —,
  // which takes a measured A/B of its own, like the unreachable solo branch of the pass waves: DESIGN.md 5.0)
  else if (n <= 8) return sweep_stats<8, SKIP, LIN, WT, BATCH>(a, L, bar, r, lf, Ssel, bb, q0, stride, nQuads, base, xcur, part, alsoPart, pw, lane, tRef, foldLf, foldA, jMax, keyLf, ctab, preS, foldD, wq, nbAll, wScale);
  else return sweep_stats<8, SKIP, LIN, WT, BATCH>(a, L, bar, r, lf, Ssel, bb, q0, stride, nQuads, base, xcur, part, alsoPart, pw, lane, tRef, foldLf, foldA, jMax, keyLf, ctab, preS, foldD, wq, nbAll, wScale);
}


// ======================================================================================== STREAMING variant (k_sweep_stream)
// Beyond 16 observations per pass thread (n > 1.04e6) the residual no longer fits the registers of the pass waves.  Same launch, same
// roles, same exchange, same redundant decisions — but the pass waves STREAM their observations per tree: residual (read + written back),
// the leaf planes of trees t-1 and t, the predictor column(s) of the two pending rules: the 22 B per observation and tree of k_tree /
// k_step, without T kernel boundaries, without a separate control kernel between two passes (k_control: 9.7 us serial per tree at
// n = 1e7) and without cold first touches of the control state.  A pass thread works through its quads in batches with a ring of loads in flight (stream_pass).
// everything one launch-step of a pass thread needs to know about the two trees in flight
struct StreamStep { int root, sset, base, prevAcc, prevRoot, prevDeath; };
// A pass thread works through its quads in batches of SW_SB quads (level-synchronous routing over the batch: the gathers of one level of
// all its observations are in flight together), a ring of three batches: two on their way while one is worked on.  Measured alternatives
// (n = 1e7, us per tree update): ring of two 82, ring of three 70.8, ring of four 74.7 (52 spilled registers); one quad at a time with
// eight quads in flight 94 (the dependent table reads of a quad are not hidden by anything: four pass waves per compute unit).
constexpr int SW_SB = 2;
struct StreamBatch { double2 r01[SW_SB], r23[SW_SB]; us4_t lf[SW_SB], pl[SW_SB], xs[SW_SB], xa[SW_SB]; };
// what the streaming loop reads of the kernel arguments, BY VALUE (the argument block itself is only reachable through an opaque pointer,
// SW_KERNARGS, and machine LICM is off for this translation unit)
struct StreamMem { double* R; const uint16_t* xbin; int64_t n, npad; int32_t* errFlag; };
template <bool APPLY, bool STATS>
__device__ __forceinline__ void stream_fetch(const StreamMem a, const uint16_t* __restrict__ lfPlane, const uint16_t* __restrict__ plPlane,
                                             const uint16_t* __restrict__ colS, const uint16_t* __restrict__ colA, bool haveS, bool haveA,
                                             int64_t qb, int64_t stride, int64_t nQuads, StreamBatch& B) {
#pragma unroll
  for (int j = 0; j < SW_SB; ++j) {
    const int64_t qd = qb + (int64_t)j * stride;
    B.r01[j] = make_double2(0.0, 0.0); B.r23[j] = make_double2(0.0, 0.0);
    B.lf[j].x = 0; B.lf[j].y = 0; B.lf[j].z = 0; B.lf[j].w = 0; B.pl[j] = B.lf[j]; B.xs[j] = B.lf[j]; B.xa[j] = B.lf[j];
    if (qd < nQuads) {
      const int64_t i0 = qd << 2;
      B.r01[j] = *reinterpret_cast<const double2*>(a.R + i0); B.r23[j] = *reinterpret_cast<const double2*>(a.R + i0 + 2);
      if (STATS) B.lf[j] = __builtin_nontemporal_load(reinterpret_cast<const us4_t*>(lfPlane + i0));
      if (APPLY) B.pl[j] = __builtin_nontemporal_load(reinterpret_cast<const us4_t*>(plPlane + i0));
      if (STATS && haveS) B.xs[j] = *reinterpret_cast<const us4_t*>(colS + i0);
      if (APPLY && haveA) B.xa[j] = *reinterpret_cast<const us4_t*>(colA + i0);
    }
  }
}
// sweep_route for ONE rule tree whose first-level predictor values are already here (xq): the byte of an observation is the binB field
// of the leaf it reaches under `root` (statistics half: its B bin; apply half, table SA: the node id itself), 0xff when its present
// leaf does not lie under `root` or `root` carries no rule.
__device__ __forceinline__ void stream_route(const StreamMem a, const NodeS* __restrict__ S, const NodeP* __restrict__ SP, int root, const us4_t (&xq)[SW_SB],
                                             const us4_t (&lf)[SW_SB], int64_t qb, int64_t stride, int64_t nQuads, unsigned (&bb)[SW_SB]) {
  const NodeP pr = SP[root];
  const int rootVar = (int)pr.var;
  unsigned insv[SW_SB][4];
#pragma unroll
  for (int j = 0; j < SW_SB; ++j) {
    const unsigned l4[4] = {lf[j].x, lf[j].y, lf[j].z, lf[j].w};
#pragma unroll
    for (int e = 0; e < 4; ++e) insv[j][e] = (unsigned)(int)S[l4[e] & 63u].insub;
  }
  const int cL = rootVar >= 0 ? (int)pr.left : 0, cR = rootVar >= 0 ? (int)pr.right : 0;
  const unsigned leafLM = sw_mask((int)SP[cL].var < 0), leafRM = sw_mask((int)SP[cR].var < 0);
  const unsigned bL = (unsigned)(int)S[cL].binB & 0xffu, bR = (unsigned)(int)S[cR].binB & 0xffu;
  const unsigned rootM = sw_mask(rootVar >= 0);
  int cur[SW_SB][4];
  unsigned anyM = 0u;
#pragma unroll
  for (int j = 0; j < SW_SB; ++j) {
    const int64_t qd = qb + (int64_t)j * stride;
    const int valid = qd < nQuads ? ((a.n - (qd << 2)) >= 4 ? 4 : (int)(a.n - (qd << 2))) : 0;
    const unsigned x4[4] = {xq[j].x, xq[j].y, xq[j].z, xq[j].w};
    unsigned packed = 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned insM = (0u - (unsigned)(insv[j][e] != 0u)) & rootM & (0u - (unsigned)(e < valid));
      const unsigned goLM = 0u - (unsigned)(x4[e] <= (unsigned)pr.cut);
      const unsigned childLeafM = sw_sel(goLM, leafLM, leafRM);
      const unsigned child = sw_sel(goLM, (unsigned)cL, (unsigned)cR);
      const unsigned deeperM = insM & ~childLeafM;
      cur[j][e] = (int)sw_sel(deeperM, child, 0xffffffffu);
      packed |= sw_sel(insM & childLeafM, sw_sel(goLM, bL, bR), 0xffu) << (8 * e);
      anyM |= deeperM;
    }
    bb[j] = packed;
  }
  int levels = 0;
  while (anyM != 0u) {    // deeper levels: change / swap moves above internal nodes (one gather per level, all observations of the batch together)
    if (++levels > 2 * S4B_MAX_DEPTH) { *a.errFlag |= S4B_ERR_INTERNAL | S4B_ERR_I_WAIT; break; }
    unsigned xv[SW_SB][4], pvc[SW_SB][4], plr[SW_SB][4];
#pragma unroll
    for (int j = 0; j < SW_SB; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { const uint2 w = *reinterpret_cast<const uint2*>(&SP[cur[j][e] >= 0 ? cur[j][e] : 0]); pvc[j][e] = w.x; plr[j][e] = w.y; }
    }
#pragma unroll
    for (int j = 0; j < SW_SB; ++j) {
      const int64_t i0 = (qb + (int64_t)j * stride) << 2;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t ie = (i0 + e) < a.npad ? (i0 + e) : 0;
        const int v = (int)(int16_t)(pvc[j][e] & 0xffffu);
        xv[j][e] = a.xbin[(size_t)(v >= 0 ? v : 0) * a.npad + (size_t)ie];
      }
    }
    anyM = 0u;
#pragma unroll
    for (int j = 0; j < SW_SB; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int raw = (xv[j][e] <= (pvc[j][e] >> 16)) ? (int)(int16_t)(plr[j][e] & 0xffffu) : (int)(int16_t)(plr[j][e] >> 16);
        const int nd = raw >= 0 ? raw : 0;
        const unsigned ndVar = (unsigned)(int)SP[nd].var, ndBin = (unsigned)(int)S[nd].binB & 0xffu;
        const unsigned actM = 0u - (unsigned)(cur[j][e] >= 0), innerM = 0u - (unsigned)((int)ndVar >= 0);
        cur[j][e] = (int)sw_sel(actM & innerM, (unsigned)nd, 0xffffffffu);
        const unsigned oldb = (bb[j] >> (8 * e)) & 0xffu;
        bb[j] = (bb[j] & ~(0xffu << (8 * e))) | (sw_sel(actM & ~innerM, ndBin, oldb) << (8 * e));
        anyM |= actM & innerM;
      }
    }
  }
}
// one batch: finish tree t-1 (APPLY: fold its leaf values into the residual, relabel under an accepted move, store) and count the batch's
// partial residuals into the bins [base, base + NB) of tree t's settled proposal (STATS)
template <int NB, bool APPLY, bool STATS>
__device__ __forceinline__ void stream_batch(const StreamMem a, const SweepLds& L, const StreamStep st, StreamBatch& B, uint16_t* __restrict__ plPlane,
                                             int64_t qb, int64_t stride, int64_t nQuads, double (&accS)[NB], int (&accN)[NB]) {
  const NodeS* __restrict__ Ssel = L.S + st.sset * SW_NC;
  unsigned bbS[SW_SB], bbA[SW_SB];
#pragma unroll
  for (int j = 0; j < SW_SB; ++j) { bbS[j] = 0xffffffffu; bbA[j] = 0xffffffffu; }
  if (APPLY && st.prevAcc && !st.prevDeath) stream_route(a, L.SA, L.AP, st.prevRoot, B.xa, B.pl, qb, stride, nQuads, bbA);
  if (STATS) stream_route(a, Ssel, L.SP + st.sset * SW_NC, st.root, B.xs, B.lf, qb, stride, nQuads, bbS);
  double rr[SW_SB][4];
#pragma unroll
  for (int j = 0; j < SW_SB; ++j) { rr[j][0] = B.r01[j].x; rr[j][1] = B.r01[j].y; rr[j][2] = B.r23[j].x; rr[j][3] = B.r23[j].y; }
  if (APPLY) {
    const unsigned accM = sw_mask(st.prevAcc != 0), deathM = sw_mask(st.prevDeath != 0);
#pragma unroll
    for (int j = 0; j < SW_SB; ++j) {
      const int64_t qd = qb + (int64_t)j * stride;
      const unsigned pl[4] = {B.pl[j].x, B.pl[j].y, B.pl[j].z, B.pl[j].w};
      double muOld[4]; unsigned ain[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) { muOld[e] = L.A[pl[e] & 63u].muOld; ain[e] = L.Ain[pl[e] & 63u]; }
      unsigned nl[4]; double muNew[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned m = (0u - (unsigned)(ain[e] != 0u)) & accM;
        nl[e] = sw_sel(m, sw_sel(deathM, (unsigned)st.prevRoot, (bbA[j] >> (8 * e)) & 0xffu), pl[e]) & 63u;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) muNew[e] = L.A[nl[e]].muNew;
#pragma unroll
      for (int e = 0; e < 4; ++e) rr[j][e] = (rr[j][e] + muOld[e]) - muNew[e];
      if (qd < nQuads) {
        const int64_t i0 = qd << 2;
        // (plain stores: this thread reads the residual back one tree later inside the same launch — a written-through store (store_r)
        // leaves the sectors this compute unit's vector cache holds from the earlier load as they were: 8 bytes of every 32 in the last 128
        // of each 512-byte block came back stale)
        *reinterpret_cast<double2*>(a.R + i0) = make_double2(rr[j][0], rr[j][1]); *reinterpret_cast<double2*>(a.R + i0 + 2) = make_double2(rr[j][2], rr[j][3]);
        if (st.prevAcc) { us4_t o4; o4.x = (unsigned short)nl[0]; o4.y = (unsigned short)nl[1]; o4.z = (unsigned short)nl[2]; o4.w = (unsigned short)nl[3];
                          __builtin_nontemporal_store(o4, reinterpret_cast<us4_t*>(plPlane + i0)); }
      }
    }
  }
  if (STATS) {
#pragma unroll
    for (int j = 0; j < SW_SB; ++j) {
      const int64_t qd = qb + (int64_t)j * stride;
      const int valid = qd < nQuads ? ((a.n - (qd << 2)) >= 4 ? 4 : (int)(a.n - (qd << 2))) : 0;
      const unsigned l4[4] = {B.lf[j].x, B.lf[j].y, B.lf[j].z, B.lf[j].w};
      NodeS ns[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) ns[e] = Ssel[l4[e] & 63u];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned okM = 0u - (unsigned)(e < valid);
        const unsigned sa = ((unsigned)(int)ns[e].binA & 0xffu) - (unsigned)st.base, sb = ((bbS[j] >> (8 * e)) & 0xffu) - (unsigned)st.base;
        const unsigned bits = ((sa < (unsigned)NB ? 1u << sa : 0u) | (sb < (unsigned)NB ? 1u << sb : 0u)) & okM;
        const double rs = e < valid ? rr[j][e] + ns[e].mu : 0.0;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          const unsigned mk = (bits >> k) & 1u;
          accS[k] = fma(__hiloint2double((int)(mk * 0x3ff00000u), 0), rs, accS[k]);
          accN[k] += (int)mk;
        }
      }
    }
  }
}
// the pass of one step over all quads of the thread, then (STATS) the block reduction of sweep_stats and the workgroup's contribution to the exchange
template <int NB, bool APPLY, bool STATS>
__device__ __forceinline__ void stream_pass(const BartArrays& a, const SweepLds& L, PassBar& bar, const StreamStep& st, int tS, int tA, int64_t q0, int64_t stride,
                                            int64_t nQuads, unsigned long long* xcur, double* part_, bool alsoPart, int pw, int lane) {
  double accS[NB]; int accN[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) { accS[k] = 0.0; accN[k] = 0; }
  const uint16_t* __restrict__ lfPlane = a.leaf + (size_t)tS * a.npad;
  uint16_t* __restrict__ plPlane = a.leaf + (size_t)tA * a.npad;
  const int rootVarS = STATS ? (int)(L.SP + st.sset * SW_NC)[st.root].var : -1;
  const int rootVarA = (APPLY && st.prevAcc && !st.prevDeath) ? (int)L.AP[st.prevRoot].var : -1;
  const uint16_t* __restrict__ colS = a.xbin + (size_t)(rootVarS >= 0 ? rootVarS : 0) * a.npad;
  const uint16_t* __restrict__ colA = a.xbin + (size_t)(rootVarA >= 0 ? rootVarA : 0) * a.npad;
  const int64_t bstride = (int64_t)SW_SB * stride;     // quads between two batches of a thread
  StreamMem m; m.R = a.R; m.xbin = a.xbin; m.n = a.n; m.npad = a.npad; m.errFlag = a.errFlag;
  auto fetch = [&](int64_t qb, StreamBatch& X) { stream_fetch<APPLY, STATS>(m, lfPlane, plPlane, colS, colA, rootVarS >= 0, rootVarA >= 0, qb, stride, nQuads, X); };
  auto work = [&](int64_t qb, StreamBatch& X) { stream_batch<NB, APPLY, STATS>(m, L, st, X, plPlane, qb, stride, nQuads, accS, accN); };
  StreamBatch A, B, C;
  fetch(q0, A); fetch(q0 + bstride, B);
  for (int64_t qb = q0; qb < nQuads; qb += 3 * bstride) {
    fetch(qb + 2 * bstride, C); work(qb, A);
    if (qb + bstride >= nQuads) break;
    fetch(qb + 3 * bstride, A); work(qb + bstride, B);
    if (qb + 2 * bstride >= nQuads) break;
    fetch(qb + 4 * bstride, B); work(qb + 2 * bstride, C);
  }
  if (!STATS) return;
  {
    const int col = pw * 64 + lane;
#pragma unroll
    for (int k = 0; k < NB; ++k) { L.redS[k * SW_RED_ROW + col] = accS[k]; L.redN[k * SW_RED_ROW + col] = accN[k]; }
  }
  pass_barrier(bar);
  if (pw == 0) {
    // (the lane id taken afresh: values derived from the one the kernel started with stay live across the whole step otherwise — in scratch
    // memory, for want of registers —, and their reloads sit on the way from the barrier to the publishing atomics)
    const int ln = sweep_fresh_lane();
    const int k = ln >> 3, part = ln & 7;
    const int kk = k < NB ? k : 0;
    double s0 = 0.0, s1 = 0.0; int c = 0;
#pragma unroll
    for (int i = 0; i < SW_PT / 8; i += 2) {
      s0 += L.redS[kk * SW_RED_ROW + i * 8 + part]; s1 += L.redS[kk * SW_RED_ROW + (i + 1) * 8 + part];
      c += L.redN[kk * SW_RED_ROW + i * 8 + part] + L.redN[kk * SW_RED_ROW + (i + 1) * 8 + part];
    }
    double sm = s0 + s1;
    sm += wave_xor<1>(sm); sm += wave_xor<2>(sm); sm += wave_xor<4>(sm);
    c += wave_xor<1>(c); c += wave_xor<2>(c); c += wave_xor<4>(c);
    if (part == 0 && k < NB) {
      if (alsoPart) {
        const size_t kind = (size_t)a.binCap * a.gridF;
        part_[(size_t)(st.base + k) * a.gridF + blockIdx.x] = sm;
        part_[kind + (size_t)(st.base + k) * a.gridF + blockIdx.x] = (double)c;
      }
      xc_publish(xcur, st.base + k, sm, c, a.errFlag);
    }
  }
}
// (the counts of a copy must fit the 21-bit field of the exchange words: fewer than 2^16 observations per pass workgroup, at most 32 pass
// workgroups per copy, i.e. n <= 16 450 560 with 255 of them; the host checks it: dev_hip.hip, streamCountOk)
template <bool APPLY, bool STATS>
__device__ __forceinline__ void stream_pass_n(int nbThis, const BartArrays& a, const SweepLds& L, PassBar& bar, const StreamStep& st, int tS, int tA, int64_t q0, int64_t stride,
                                              int64_t nQuads, unsigned long long* xcur, double* part, bool alsoPart, int pw, int lane) {
  if (nbThis <= 4) stream_pass<4, APPLY, STATS>(a, L, bar, st, tS, tA, q0, stride, nQuads, xcur, part, alsoPart, pw, lane);
  else stream_pass<8, APPLY, STATS>(a, L, bar, st, tS, tA, q0, stride, nQuads, xcur, part, alsoPart, pw, lane);
}

template <bool STREAM, bool FEW, bool SPL = false, bool WT = false, bool BATCH = false, class AK = BartArrays, class XK = SweepArgs>
__device__ __forceinline__ void sweep_body(AK aKern, XK xKern) {      // (BATCH: AK / XK are placeholders, the arguments come from the member's slot)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ ControlShared S;
  __shared__ SweepShared F;
  __shared__ SweepModel M;
  __shared__ double spTab[SPL ? SP_TAB : 1];      // (cgm(split.probs): WaveModelT<true>, dev_control.hpp)
  __shared__ __attribute__((aligned(16))) double wLds[WT ? SW_PT * SW_PF * 4 : 2];      // (observation weights of the workgroup's observations: sweep_stats<.., WT>)
  constexpr int NBX = WT ? 2 : 1;      // "bins" a step exchanges per bin of its statistics (the sums of the weights travel as bins of their own)
  static_assert(!(WT && STREAM), "no weighted streaming sweep"); static_assert(!(BATCH && STREAM), "the streaming sweep is never solo");
  (void)xKern; (void)spTab; (void)wLds;
  // waits: k_sweep's steps are ~10 us of dependent hand-overs — its control waves poll every 64 cycles at raised priority; a step of the
  // streaming variant is dominated by the pass (tens of us), during which every control wave of the workgroup only waits: there they
  // sleep 512 cycles between polls and keep the default priority, or their polling takes a third of the issue slots of the pass waves
  constexpr int SW_SLEEP = STREAM ? 8 : 1;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  constexpr int MTW = (int)(sizeof(MTState) / 4), MTJ = (MTW + 63) / 64;
  int T_ = 0; if constexpr (BATCH) { SW_KERNARGS(); T_ = a.T; } else T_ = aKern.T; const int T = T_;      // (BATCH: T from the member's slot)
  // SOLO (gridDim.x == 1, at most SW_PT * SW_PF quads = 4096 observations): one workgroup holds every observation AND the control
  // duties; the bin totals never leave the chip — wave 4's reduction IS the total, no exchange words, no polling (a tree update then
  // costs what the decision and the pass cost, not a trip through memory)
  const bool solo = SW_GX == 1;
  const int NP = solo ? 1 : (int)SW_GX - 1;   // workgroups with observations
  const bool ctl = solo || (int)SW_BX == NP; // writes the decided trees / the trace to the main arrays
  const bool hasObs = solo || (int)SW_BX < NP;
  const SweepLds L = carve_sweep(smem);
  {
    SW_KERNARGS();
    // ---- does the first control step fit the wave path at all?  (same answer in every workgroup)
    {
      const int hwm0 = a.hwm[0];
      if (!step_fits_wave(hwm0 + 2, 0, a.nc)) {
        // (nothing of this launch's ring is touched, but the ring of the next launch — the one the launch before this one used — is
        // cleared as always: the next persistent launch finds it armed)
        if (ctl) { for (int i = threadIdx.x; i < XC_RING_WORDS + XC_ROLL_WORDS; i += FBLOCK) x.xnext[i] = 0ull; if (threadIdx.x == 0) *x.status = 0; }
        return;
      }
    }
    // ---- ROLL CALL: is every workgroup of this launch resident?  The workgroups wait for each other inside the sweep, so a launch
    // that shares the device with somebody else's kernel (another process: the per-device lock of the host side cannot see it) must not
    // start on a part of its grid.  Before anything is written: every workgroup takes a ticket; the last one to arrive says GO, a
    // workgroup that has waited SW_ROLL_TICKS without seeing a decision says BUSY — one compare-and-swap decides for everybody, also for
    // the workgroups that only start once compute units have become free.  BUSY leaves the chain exactly as it was: the host runs this
    // sweep with k_step launches and comes back to the persistent launch later (DevHip::sweep_persistent_finish).
    if (!solo) {
      unsigned long long* const roll = x.xbuf + (size_t)XC_RING_WORDS;     // [0] tickets, [1] decision: two words behind the ring, cleared with it
      if (threadIdx.x == 0) {
        const unsigned long long k = __hip_atomic_fetch_add(roll, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned long long w = 0ull;
        if (k + 1 == (unsigned long long)SW_GX) { unsigned long long z = 0ull; __hip_atomic_compare_exchange_strong(roll + 1, &z, SW_ROLL_GO, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
        const long long t0 = wall_clock64();
        while ((w = __hip_atomic_load(roll + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0ull) {
          __builtin_amdgcn_s_sleep(4);
          if (wall_clock64() - t0 > SW_ROLL_TICKS) { unsigned long long z = 0ull; __hip_atomic_compare_exchange_strong(roll + 1, &z, SW_ROLL_BUSY, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
        }
        F.last = (int)w;
      }
      __syncthreads();
      if (F.last != (int)SW_ROLL_GO) {
        if (ctl) {   // (the ring of the next launch is cleared as always: that launch holds its own roll call in it)
          for (int i = threadIdx.x; i < XC_RING_WORDS + XC_ROLL_WORDS; i += FBLOCK) x.xnext[i] = 0ull;
          if (threadIdx.x == 0) *x.status = -2;
        }
        return;
      }
      __syncthreads();
    }
    // ---- prologue: on-chip copies of what the whole sweep reads
    if (threadIdx.x < 64) {
      const int l = threadIdx.x;
      M.pg[l] = a.model.pgDepth[l]; M.lpg[l] = a.model.logPg[l]; M.l1pg[l] = a.model.log1mPg[l];
      M.li0[l] = l < a.model.logIntLen ? a.model.logInt[l] : 0.0; M.li1[l] = 64 + l < a.model.logIntLen ? a.model.logInt[64 + l] : 0.0;
      M.nc0[l] = l < a.P ? a.numCuts[l] : 0; M.nc1[l] = 64 + l < a.P ? a.numCuts[64 + l] : 0;
      if (l == 0) M.sigma = a.scale->sigma;
    }
    for (int i = threadIdx.x; i < MTW; i += FBLOCK) ((uint32_t*)&S.rng[0])[i] = ((const uint32_t*)a.rngF)[i];
    // every table entry finite and every index table in range from the start: table reads are unconditional (observation slots
    // beyond n read entry 0, a B bin "none" reads b2n[63]), and 0 x NaN is NaN even where the factor says "not in this bin"
    for (int i = threadIdx.x; i < SW_SETS * SW_NC * 4; i += FBLOCK) ((int*)L.S)[i] = 0;
    for (int i = threadIdx.x; i < SW_SETS * SW_NC * 2; i += FBLOCK) ((int*)L.SP)[i] = 0;
    for (int i = threadIdx.x; i < 2 * SW_NC * 4; i += FBLOCK) ((int*)L.A)[i] = 0;
    for (int i = threadIdx.x; i < 32; i += FBLOCK) { ((int*)L.Ain)[i & 15] = 0; ((int*)L.b2n)[i & 15] = 0; }
    for (int i = threadIdx.x; i < 2 * SW_CT_WORDS; i += FBLOCK) L.ctab[i] = 0u;
    for (int i = threadIdx.x; i < SW_NC * 4; i += FBLOCK) ((int*)L.zeroA)[i] = 0;
    if (threadIdx.x < 2 * SW_PW * 8) L.preS[threadIdx.x] = 0.0;
    if (threadIdx.x < 16) L.preC[threadIdx.x] = 0;
    if (threadIdx.x < 2 * SW_NC) L.dtab[threadIdx.x] = 0.0;
    if (threadIdx.x < 64) F.tacc[threadIdx.x] = 0ull;
    if (threadIdx.x == 0) {
      S.arrived = 0; S.verdict = 0;
      F.prevAcc = 0; F.prevRoot = 0; F.prevDeath = 0; F.root = 0; F.nb = 0; F.needBig = 0; F.sset = 0; F.paType = 0; F.paStatus = 0; F.paNbA = 0;
      F.selSlot[0] = 0; F.selSlot[1] = 0; F.paGo = 0; F.foldReady = 0; F.tablesReady = 0; F.rng0Copied = -1; F.rng1Copied = -1; F.img0Ready = 0; F.img1Ready = 0; F.pre0Copied = 0; F.staged = 0; F.bar = 0; F.published = 0; F.abort = 0; F.last = 0; F.specReady = 0; F.specNb[0] = 0; F.specNb[1] = 0; F.publishedAlt = 0; F.passSeen = 0; F.specCnt = 0; F.decDone = 0; F.bothStep = -1;
      F.linReady = 0; F.pre0Ready = 0; F.aheadId[0] = 0; F.aheadId[1] = 0; F.aheadId[2] = 0; F.aheadNb[0] = 0; F.aheadNb[1] = 0; F.aheadNb[2] = 0; F.preDoneA = 0; F.preDoneB = 0; F.preArrA = 0; F.preArrB = 0; F.statArr = 0; F.preNb[0] = 0; F.preNb[1] = 0; F.preSeq[0] = 0; F.preSeq[1] = 0;
      // (the ticket word is the target of agent-scope atomics of OTHER workgroups at the end of a handed-over launch: a plain store
      // here would sit in this XCD's L2 and be written back over their increments — fuzz seed 2576: both workgroups drew ticket 0)
      if (ctl) { __hip_atomic_store(a.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); a.preDone[0] = 0; a.preDone[1] = 0; }
    }
    if (threadIdx.x < 3) cand_lds(L.img, (int)threadIdx.x, 0).meta[0] = 0; else if (threadIdx.x < 5) cand_lds(L.img, (int)threadIdx.x - 3, 1).meta[0] = 0;
    // the control workgroup clears the exchange ring of the NEXT launch (nobody touches it during this one; the kernel boundary
    // publishes the stores): no memset between launches
    if (ctl) for (int i = threadIdx.x; i < XC_RING_WORDS + XC_ROLL_WORDS; i += FBLOCK) x.xnext[i] = 0ull;
    if (wv == 4) stage_tree(a, L.stage, 0, lane);
    if constexpr (SPL) { if (wv == 5) wave_fill_sp_tab(a, spTab, lane); }
    if constexpr (WT) {
      if (wv >= 4) {      // pass thread pt keeps the weights of its quads j at wLds[(j * SW_PT + pt) * 4 ..]; 0 beyond n
        const int ptW = (wv - 4) * 64 + lane;
        const int64_t nQuadsW = (a.n + 3) >> 2;
#pragma unroll
        for (int j = 0; j < SW_PF; ++j) {
          const int64_t qd = (int64_t)SW_BX * SW_PT + ptW + (int64_t)j * NP * SW_PT;
#pragma unroll
          for (int e = 0; e < 4; ++e) { const int64_t i = (qd << 2) + e; wLds[((size_t)j * SW_PT + ptW) * 4 + e] = (hasObs && qd < nQuadsW && i < a.n) ? a.wts[i] : 0.0; }
        }
      }
    }
  }
  __syncthreads();
  int bailStep = -1;      // >= 0: the launch ends after this step (the next control step does not fit the wave path)
#ifdef S4B_SWEEP_TIMING
  long long tStep = wall_clock64();
#endif

  // Priorities.  The control roles are dependent chains of wave-uniform code that share their SIMDs with the pass waves' bulk arithmetic.  Until round 5
  // they went first (3 against 0).  Since the statistics are published before the verdict the chain of a step is totals -> wave 3's leaf values ->
  // speculative statistics -> exchange: the exchange wave stays on top, the pass waves run their speculative statistics above the decider and the
  // image waves, which have microseconds of slack per step (S4B_PRIO_*, measured: 3 / 3 / 3 / 0 -> 423 it/s, 1 / 1 / 3 / 2 and 2 / 0 / 3 / 3 -> 438 - 445, 0 / 0 / 3 / 3 -> 435)
  if (!STREAM) { if (wv == 0) __builtin_amdgcn_s_setprio(S4B_PRIO_DEC); else if (wv == 3) __builtin_amdgcn_s_setprio(S4B_PRIO_XCH); else if (wv < 3) __builtin_amdgcn_s_setprio(S4B_PRIO_IMG); }
  if (wv == 0) {
    // ====================================================================================== wave 0: the decider
    for (int t = 0; t <= T; ++t) {
      const bool doDecide = t > 0, doPropose = t < T;
      const int tt = doDecide ? t - 1 : 0, tn = doPropose ? t : 0;
      const int tnn = t + 1 < T ? t + 1 : tn;
      const bool ahead = doPropose && t + 1 < T;
      const bool spec = doDecide && doPropose;
      SW_KERNARGS();
      const int nc = a.nc;
      const bool laneIn = lane < nc;
      WaveModelT<SPL> m;
      static_cast<ModelView&>(m) = a.model;
      m.scratch = S.scratch[0];
      m.pg.load(M.pg[lane]); m.lpg.load(M.lpg[lane]); m.l1pg.load(M.l1pg[lane]); m.li0.load(M.li0[lane]); m.li1.load(M.li1[lane]);
      m.nc0 = M.nc0[lane]; m.nc1 = M.nc1[lane];
      if constexpr (SPL) m.spTab = spTab;
      const int selT = __builtin_amdgcn_readfirstlane(F.selSlot[tt & 1]);
      const CandSet cs = cand_lds(L.img, tt, selT);
      NodeA* const At = L.A + (STREAM ? 0 : (t & 1)) * SW_NC;      // leaf-value table of this step
      const TreeStage* stN = L.stage + (tn % SW_STAGES);
      if (doDecide && doPropose) spin_counter(&F.staged, t, &F.abort);    // wave 4 staged tree tn during the previous step (long ago — but nothing else orders it before this wave's reads)
      WaveTree curT; WaveTables tbT; WaveCache caT; WaveArrD mu, muOld; WaveArr<int32_t> cnt;
      mu.load(0.0); muOld.load(0.0); cnt.r = 0;
      StepScalars g;
      {
        int w = 0;
        if (lane < 28) w = doDecide ? ((const int32_t*)cs.head)[lane] : 0;
        else if (lane >= 40 && lane < 40 + TI_COUNT) w = stN->sc[lane - 40];
        g.w = w;
        const double d = lane == 1 ? stN->logPi : (lane == 2 ? M.sigma : 0.0);
        g.dlo = __double2loint(d); g.dhi = __double2hiint(d);
      }
      const int ncW = nc < 64 ? nc : 64;
      if (doDecide) {
        const int16_t* sT = cs.slab;
        curT.var.r = sT[SF_CVAR * SW_NC + lane]; curT.cut.r = ((const uint16_t*)sT)[SF_CCUT * SW_NC + lane]; curT.left.r = sT[SF_CLEFT * SW_NC + lane];
        curT.right.r = sT[SF_CRIGHT * SW_NC + lane]; curT.parent.r = sT[SF_CPARENT * SW_NC + lane]; curT.na.r = sT[SF_CNA * SW_NC + lane];
        curT.dep.r = sT[SF_CDEP * SW_NC + lane]; curT.nc = ncW;
        tbT.prop.var.r = sT[SF_VAR * SW_NC + lane]; tbT.prop.cut.r = ((const uint16_t*)sT)[SF_CUT * SW_NC + lane]; tbT.prop.left.r = sT[SF_LEFT * SW_NC + lane];
        tbT.prop.right.r = sT[SF_RIGHT * SW_NC + lane]; tbT.prop.parent.r = sT[SF_PARENT * SW_NC + lane]; tbT.prop.na.r = sT[SF_NA * SW_NC + lane];
        tbT.prop.dep.r = sT[SF_DEP * SW_NC + lane]; tbT.prop.nc = ncW;
        tbT.binA.r = sT[SF_BINA * SW_NC + lane]; tbT.binB.r = sT[SF_BINB * SW_NC + lane]; tbT.insub.r = cs.insub[lane]; tbT.list.r = 0;
        caT.leaf.r = sT[SF_CLEAF * SW_NC + lane]; caT.pre.r = sT[SF_CPRE * SW_NC + lane]; caT.post.r = sT[SF_CPOST * SW_NC + lane];
        mu.load(cs.snapMu[lane]); cnt.r = cs.snapCnt[lane];
      }
      Proposal prT; g.proposal(prT);
      if (!doDecide) { prT.type = MOVE_CHANGE; prT.status = -1; prT.nbA = 0; prT.nbB = 0; prT.hwm = 0; prT.node = 0; }
      const int hwmT = doDecide ? g.i32(20) : 0, hwmN = g.i32(40 + TI_HWM);
      int need = 0, nb = 0;
      if (doDecide) { need = prT.hwm > hwmT ? prT.hwm : hwmT; nb = prT.nbA + prT.nbB; }
      if (doPropose && hwmN + 2 > need) need = hwmN + 2;
      if (!step_fits_wave(need, NBX * nb, nc) && lane == 0) *a.errFlag |= S4B_ERR_INTERNAL | S4B_ERR_I_FITS;   // the previous step should have ended the launch
      MTState* const stream = doDecide ? cs.rng : &S.rng[0];     // decide(t-1) continues the stream the surviving image of t-1 left behind
      WaveRng rng; rng.st = stream; rng.mti = 0; rng.wbase = -64; rng.win = 0u; rng.count = 0; rng.regen = 0;
      auto openRng = [&]() {
        if (doDecide) { spin_counter(&F.rng0Copied, tt, &F.abort); spin_counter(&F.rng1Copied, tt, &F.abort); }   // the image waves have their copies of this generator: the state may move on in place
        rng.open(stream);
      };
      int winner = 0;
      bool didDecide = false; int dHwmNew = 0, dCntOut = 0; int32_t dAccepted = 0;
      StepRecord dRec; dRec.type = 0; dRec.status = 0; dRec.var = 0; dRec.split = 0; dRec.numLeaves = 0;
      if (!doDecide) openRng();
      if (doDecide) {
        caT.nl = g.i32(21); caT.ni = g.i32(22); caT.g = g.i32(23); caT.gn = g.i32(24); caT.valid = 1;
        caT.logPi = g.f64w(26);
        const double sigma = g.f64(2);
        spin_counter(&S.arrived, t, &F.abort);
        SW_T(9); SW_A(41); SW_ABS(0);
        WaveArrD binSum, binCnt;
        { double sSum = 0.0, sCnt = 0.0;
          if (lane < nb) { sSum = F.totS[lane]; sCnt = F.totC[lane]; }
          binSum.load(sSum); binCnt.load(sCnt); }
        WaveArrD binWt = binCnt;
        if constexpr (WT) binWt.load(lane < nb ? F.totS[nb + lane] : 0.0);      // (the sums of the weights: "bins" nb .. 2 nb - 1 of the exchange)
        DecideWork<WaveArrD> wk;
        wk.ll.load(0.0); wk.lc.load(0.0); wk.ls.load(0.0); wk.u1.load(0.5); wk.u2.load(0.5); wk.val.load(0.0); wk.lw.load(0.0);
        StepRecord rec; int32_t accepted = 0;
        bool earlyDone = false; int earlyUsed = 0;
        // what the pass waves wait for, part 1: which image of tree tn survives (`used` draws consumed), old leaf values, relabelling tables
        auto publish = [&](int used, int acc) {
          int v0 = 0, h0 = 0, v1 = 0, h1 = 0;
          if (spec) {
            spin_counter(&F.img0Ready, tn, &F.abort);
            const int32_t* m0 = cand_lds(L.img, tn, 0).meta;
            v0 = S4B_UNI(m0[0]); h0 = S4B_UNI(m0[1]);
            // (round 6: image 1 — an accepted birth / death of the tree before — is only waited for when image 0 is not the one: its drawing, 1.5 - 4 us on
            // wave 2, sat between two verdicts in every step although 98 % of the steps of a stationary chain never look at it)
            if (!(v0 && used == h0)) {
              spin_counter(&F.img1Ready, tn, &F.abort);
              const int32_t* m1 = cand_lds(L.img, tn, 1).meta;
              v1 = S4B_UNI(m1[0]); h1 = S4B_UNI(m1[1]);
            }
          }
          winner = (v0 && used == h0) ? 1 : ((v1 && used == h1) ? 2 : 0);
          // (the pass waves publish before the verdict when they speculate: the totals of this step may be complete, and this wave here, while
          // they still read what the decision of the PREVIOUS step left for them — flags, tables, the settled proposal, which the image waves
          // overwrite at the verdict —: all of it may go once they are through)
          if constexpr (!STREAM) spin_counter(&F.passSeen, 4 * t, &F.abort);
          // (the verdict lets an image wave — or this wave — settle the proposal of tree t: F.root .. F.paNbA, one set of words.  Both image waves must have read what
          // the step before settled there — they have once they hold their copy of that tree's generator.  Until round 6 the wait for image 1 above kept wave 2 within
          // a step of this wave; without it a lagging wave 2 read the NEXT tree's words and drew its image from the wrong source: one chain in five differed)
          if (doDecide) { spin_counter(&F.rng0Copied, tt, &F.abort); spin_counter(&F.rng1Copied, tt, &F.abort); }
          if (lane == 0) __hip_atomic_store(&S.verdict, (t << 2) | (winner ? winner : 3), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
          // first half of the apply tables — everything but the new leaf values, which the leaf arithmetic below produces: old
          // value per node, "the observation moves" flags, and for an accepted move the node behind every B bin (where the
          // observations counted in it go).  The pass waves fold the old values in and relabel while this wave draws the leaves.
          {
            const int cnt0 = prT.hwm > hwmT ? prT.hwm : hwmT;
            // (wave 3 writes whole records — old and early new value — of the leaves: it is through before this wave's old values go in)
            { int guard = 0; while ((__hip_atomic_load(&F.specReady, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) >> 1) < t) { __builtin_amdgcn_s_sleep(SW_SLEEP); if (++guard > (1 << 21)) { F.abort = __LINE__; break; } } }
            if (lane < cnt0) {
              At[lane].muOld = muOld.mine(); L.Ain[lane] = (uint8_t)tbT.insub.r;
              const int bB = (int)(int16_t)tbT.binB.r;
              if (bB >= 0) L.b2n[bB & 63] = (uint8_t)lane;
              if (STREAM) {   // the decided tree as proposed, for the apply-half routing of the streaming pass (read only under an accepted move)
                NodeP p; p.var = (int16_t)tbT.prop.var.r; p.cut = (uint16_t)tbT.prop.cut.r; p.left = (int16_t)tbT.prop.left.r; p.right = (int16_t)tbT.prop.right.r;
                NodeS sa; sa.mu = 0.0; sa.binA = -1; sa.binB = (int16_t)lane; sa.insub = (int16_t)tbT.insub.r; sa.pad = 0;
                L.AP[lane] = p; L.SA[lane] = sa;
              }
            }
            if (lane == 0) { F.prevAcc = acc; F.prevRoot = prT.node; F.prevDeath = prT.type == MOVE_DEATH ? 1 : 0; }
#ifdef S4B_SWEEP_TIMING
            if (lane == 0) F.tFold = wall_clock64();
#endif
            if (lane == 0) __hip_atomic_store(&F.foldReady, t, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
          }
          SW_A(42); SW_ABS(3);
        };
        // The common outcome — the move is NOT accepted (or there is none) — leaves the tree as it is: its leaf values depend on nothing
        // the accept test produces.  Wave 3 computes them beside this wave's likelihood arithmetic (same statistics, same stream
        // positions, same arithmetic: bit-identical) and puts them into A[].muNew; when the test then says "no", everything the pass
        // waves wait for goes out at once.  This wave still draws the leaves itself afterwards (its own state; checked against wave 3's).
        auto early = [&](int acc) -> bool {
          if (acc) return false;
          int guard = 0, sp;
          while (((sp = __hip_atomic_load(&F.specReady, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) >> 1) < t) {
            __builtin_amdgcn_s_sleep(SW_SLEEP);
            if (++guard > (1 << 21)) { F.abort = __LINE__; return false; }
          }
          if (!(sp & 1)) return false;
          SW_ABS(1);
          const int nNe = __builtin_amdgcn_readfirstlane(F.specCnt);
          earlyUsed = rng.count + 2 * nNe;
          if constexpr (!STREAM) spin_counter(&F.passSeen, 4 * t, &F.abort);      // (see publish)
          SW_ABS(2);
          if (lane == 0) F.bothStep = t;
          publish(earlyUsed, 0);
          if (lane == 0) __hip_atomic_store(&F.tablesReady, t, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
          earlyDone = true;
          SW_T(10); SW_T(11); SW_A(43);
#ifdef S4B_SWEEP_TIMING
          if ((int)SW_BX == SW_TIMED_WG && lane == 0 && t > 0 && t < T) atomicAdd(&F.tacc[35], 1ull);
#endif
          // wave 3's values ARE the leaf values (same statistics, same stream positions, same arithmetic): this wave takes them over instead
          // of drawing them again — the generator moves past their uniforms (no block renewal among them: wave 3's `valid`), node n's lane
          // takes the count of its A bin and the value from the table
          rng.mti += 2 * nNe; rng.count += 2 * nNe; rng.wbase = -64;
          {
            const int bA = (int)(int16_t)tbT.binA.r;
            const double c = wave_gather(bA & 63, binCnt);
            if (bA >= 0 && lane < hwmT) { cnt.r = (int32_t)c; mu.load(At[lane].muNew); }
          }
          return true;
        };
        auto post = [&]() {   // the draws are counted: which image of tree tn (if any) was drawn from the position they leave behind?
          if (earlyDone) { if (rng.count != earlyUsed && lane == 0) *a.errFlag |= S4B_ERR_INTERNAL | S4B_ERR_I_FITS; return; }
          publish(rng.count, accepted);
          SW_T(10);
        };
        const int hwmNew = decide(curT, mu, cnt, muOld, hwmT, m, sigma, &rng, &prT, tbT, binCnt, binSum, binWt, wk, &accepted, &rec, caT, post, ctl, openRng, early);
        const int cntOut = prT.hwm > hwmNew ? prT.hwm : hwmNew;
        didDecide = true; dHwmNew = hwmNew; dCntOut = cntOut; dAccepted = accepted; dRec = rec;
        if (!earlyDone) {
          // second half of the apply tables: the new leaf values (after wave 3 has left the table alone)
          { int guard = 0; while ((__hip_atomic_load(&F.specReady, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) >> 1) < t) { __builtin_amdgcn_s_sleep(SW_SLEEP); if (++guard > (1 << 21)) { F.abort = __LINE__; break; } } }
          if (lane < cntOut) At[lane].muNew = mu.mine();
          if (lane == 0) __hip_atomic_store(&F.tablesReady, t, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
          SW_T(11); SW_A(43);
        }
        if (lane == 0) __hip_atomic_store(&F.decDone, t, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        SW_G(95); SW_ABS(4);
      } else if (lane == 0) __hip_atomic_store(&S.verdict, (t << 2) | 3, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (!doPropose) {
        rng.close();
        if (ctl) {   // the stream ends here: back to slot 0, where it lives between sweeps
#pragma unroll
          for (int j = 0; j < MTJ; ++j) { const int i = lane + j * 64; if (i < MTW) ((uint32_t*)a.rngF)[i] = ((const uint32_t*)stream)[i]; }
          if (lane == 0) a.rngF->pad = 0;
        }
      }
      if (doPropose && winner == 0) {
        // ============================================================ proposal of tree tn by wave 0 itself (start of a sweep; no image fits the draws)
        WaveTree curN; WaveCache caN; WaveTables tbN; WaveArrD muN; int cntN = 0;
        curN.nc = ncW;
        curN.var.r = laneIn ? (int)stN->row[TF_VAR][lane] : (int)NODE_FREE; curN.cut.r = (int)(uint16_t)stN->row[TF_CUT][lane]; curN.left.r = stN->row[TF_LEFT][lane];
        curN.right.r = stN->row[TF_RIGHT][lane]; curN.parent.r = stN->row[TF_PARENT][lane]; curN.na.r = stN->row[TF_NA][lane]; curN.dep.r = stN->row[TF_DEP][lane];
        caN.leaf.r = stN->row[TF_LEAF][lane]; caN.pre.r = stN->row[TF_PRE][lane]; caN.post.r = stN->row[TF_POST][lane];
        muN.load(stN->mu[lane]); cntN = stN->cnt[lane];
        caN.nl = g.i32(40 + TI_NL); caN.ni = g.i32(40 + TI_NI); caN.g = g.i32(40 + TI_G); caN.gn = g.i32(40 + TI_GN); caN.valid = g.i32(40 + TI_VALID);
        caN.logPi = g.f64(1);
        if (!caN.valid) tv_rebuild_cache(curN, m, caN);
        tbN.prop = curN;
        tbN.binA.r = -1; tbN.binB.r = -1; tbN.insub.r = 0; tbN.list.r = 0;
        Proposal prN;
        const int perr = propose(curN, hwmN, m, &rng, &prN, tbN, caN);
        rng.close();
        if (lane < prN.hwm) {   // statistics half of the pass: table set 0
          NodeS s; s.mu = muN.mine(); s.binA = (int16_t)tbN.binA.r; s.binB = (int16_t)tbN.binB.r; s.insub = (int16_t)tbN.insub.r; s.pad = 0;
          NodeP p; p.var = (int16_t)tbN.prop.var.r; p.cut = (uint16_t)tbN.prop.cut.r; p.left = (int16_t)tbN.prop.left.r; p.right = (int16_t)tbN.prop.right.r;
          L.S[lane] = s; L.SP[lane] = p;
        }
        int needNext = prN.hwm > hwmN ? prN.hwm : hwmN;
        if (ahead) { spin_counter(&F.staged, t + 1, &F.abort); const int hwmNN = S4B_UNI(L.stage[tnn % SW_STAGES].sc[TI_HWM]); if (hwmNN + 2 > needNext) needNext = hwmNN + 2; }
        const int big = step_fits_wave(needNext, NBX * (prN.nbA + prN.nbB), nc) ? 0 : 1;
        // the image the next step decides from: the slot of image 0 of this tree (both images of it are dead: the verdict is out, their
        // waves have everything they need of them in registers — wave 1 also what it took from image 0 to draw the next tree's ahead)
        if (spec) { spin_counter(&F.img0Ready, tn, &F.abort); spin_counter(&F.img1Ready, tn, &F.abort); spin_counter(&F.pre0Copied, tn, &F.abort); }
        {
          const CandSet cd = cand_lds(L.img, tn, 0);
          int16_t* const sO = cd.slab;
          const int cntOut = prN.hwm;
          wave_tree_store(tbN.prop, sO + SF_VAR * SW_NC, (uint16_t*)(sO + SF_CUT * SW_NC), sO + SF_LEFT * SW_NC, sO + SF_RIGHT * SW_NC, sO + SF_PARENT * SW_NC, cntOut, lane);
          if (lane < cntOut) { sO[SF_BINA * SW_NC + lane] = (int16_t)tbN.binA.r; sO[SF_BINB * SW_NC + lane] = (int16_t)tbN.binB.r; cd.insub[lane] = (uint8_t)tbN.insub.r;
                               sO[SF_NA * SW_NC + lane] = (int16_t)tbN.prop.na.r; sO[SF_DEP * SW_NC + lane] = (int16_t)tbN.prop.dep.r; }
          sO[SF_CVAR * SW_NC + lane] = (int16_t)curN.var.r; ((uint16_t*)sO)[SF_CCUT * SW_NC + lane] = (uint16_t)curN.cut.r; sO[SF_CLEFT * SW_NC + lane] = (int16_t)curN.left.r;
          sO[SF_CRIGHT * SW_NC + lane] = (int16_t)curN.right.r; sO[SF_CPARENT * SW_NC + lane] = (int16_t)curN.parent.r; sO[SF_CNA * SW_NC + lane] = (int16_t)curN.na.r;
          sO[SF_CDEP * SW_NC + lane] = (int16_t)curN.dep.r; sO[SF_CLEAF * SW_NC + lane] = (int16_t)caN.leaf.r; sO[SF_CPRE * SW_NC + lane] = (int16_t)caN.pre.r;
          sO[SF_CPOST * SW_NC + lane] = (int16_t)caN.post.r; cd.snapMu[lane] = muN.mine(); cd.snapCnt[lane] = cntN;
          step_header_store(prN, hwmN, caN.nl, caN.ni, caN.g, caN.gn, caN.logPi, cd.head, lane);
#pragma unroll
          for (int j = 0; j < MTJ; ++j) { const int i = lane + j * 64; if (i < MTW) ((uint32_t*)cd.rng)[i] = ((const uint32_t*)stream)[i]; }
          if (lane < 4) cd.meta[lane] = lane == 0 ? 1 : (lane == 1 ? 0 : (lane == 2 ? perr : (0x40000000 | t)));     // ([3]: drawing number — never one of the image waves')
        }
        if (perr != 0 && lane == 0 && ctl) *a.errFlag |= S4B_ERR_NODE_CAPACITY;
        if (lane == 0) { F.root = prN.node; F.nb = prN.nbA + prN.nbB; F.needBig = big; F.sset = 0; F.selSlot[tn & 1] = 0;
                         F.paType = prN.type; F.paStatus = prN.status; F.paNbA = prN.nbA; }
        if (lane == 0) __hip_atomic_store(&F.paGo, t + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      // global write-backs (control workgroup only; nobody reads these before the next sweep)
      if (ctl && didDecide) {
        int16_t* const tI = a.treeI16; int32_t* const tS = a.treeI32;
        const size_t ts = (size_t)T * nc, oT = (size_t)tt * nc, tT = (size_t)T;
        wave_tree_store(curT, tI + TF_VAR * ts + oT, (uint16_t*)(tI + TF_CUT * ts + oT), tI + TF_LEFT * ts + oT, tI + TF_RIGHT * ts + oT,
                        tI + TF_PARENT * ts + oT, dCntOut, lane);
        if (lane < dCntOut) { a.mu[oT + lane] = mu.mine(); a.cnt[oT + lane] = cnt.r; tI[TF_NA * ts + oT + lane] = (int16_t)curT.na.r; tI[TF_DEP * ts + oT + lane] = (int16_t)curT.dep.r; }
        if (laneIn) { tI[TF_LEAF * ts + oT + lane] = (int16_t)caT.leaf.r; tI[TF_PRE * ts + oT + lane] = (int16_t)caT.pre.r; tI[TF_POST * ts + oT + lane] = (int16_t)caT.post.r; }
        if (lane == 0) {
          tS[TI_HWM * tT + tt] = dHwmNew; tS[TI_NL * tT + tt] = caT.nl; tS[TI_NI * tT + tt] = caT.ni; tS[TI_G * tT + tt] = caT.g; tS[TI_GN * tT + tt] = caT.gn;
          tS[TI_VALID * tT + tt] = 1; a.clogpi[tt] = caT.logPi;
          *a.sc[tt & 1].accepted = dAccepted;
          if (a.traceOn) push_trace(a, dRec);
        }
      }
      SW_T(12); SW_MARK();
      if (__hip_atomic_load(&F.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
      if (doPropose) {
        spin_counter(&F.paGo, t + 1, &F.abort);
        if (__builtin_amdgcn_readfirstlane(F.needBig)) { bailStep = t; break; }
      }
    }
  } else if (wv <= 2) {
    // ====================================================================================== waves 1, 2: the image waves
    // Wave 1 owns image 0 of every tree (the proposal drawn from the generator position a NOT accepted decide of the tree before leaves
    // behind: 77 % of the steps of a cold chain, 98 % of a stationary one), wave 2 image 1 (an accepted birth / death before it).  Image 0
    // is drawn one step AHEAD: as soon as image 0 of tree t+1 is final, wave 1 draws image 0 of tree t+2 from it, assuming it survives; when
    // decide(t) then settles tree t+1 on anything else, that image is drawn again from the survivor (what every step did before round 5).
    // The chain of proposal drawings (1.3 - 9 us each in a stationary chain) thereby runs a step ahead of the decisions instead of between
    // them, and the pass waves route under image 0 only (an accepted birth / death routes after its verdict).
    const int candIdx = wv - 1;
    int pre = -1;            // (wave 1) tree whose image 0 sits in its slot drawn ahead, from image 0 of the tree before it
    int drawNo = 0;          // drawings of this wave so far: every image carries the number of its drawing (meta[3]) — statistics gathered ahead under an image are only used for that very drawing
    for (int t = 0; t < T; ++t) {
      const bool doDecide = t > 0;
      const int tn = t, tnn = t + 1 < T ? t + 1 : tn;
      const bool ahead = t + 1 < T;
      const bool spec = doDecide;
      SW_KERNARGS();
      const int nc = a.nc;
      // ---- this wave's image of tree tn: does it survive the verdict of decide(t-1)?  Then it settles the proposal of tree tn.
      if (spec) {
        const CandSet cd = cand_lds(L.img, tn, candIdx);
        // (this wave wrote the image itself, in an earlier step: program order)
        const int hw = lane < 28 ? ((const int32_t*)cd.head)[lane] : (lane < 31 ? cd.meta[lane - 28] : 0);
        const int valid = __builtin_amdgcn_readlane(hw, 28);
        if (valid) {
          const int pType = __builtin_amdgcn_readlane(hw, 0), pStatus = __builtin_amdgcn_readlane(hw, 1), pNode = __builtin_amdgcn_readlane(hw, 2);
          const int pNbA = __builtin_amdgcn_readlane(hw, 5), pNbB = __builtin_amdgcn_readlane(hw, 6), pHwm = __builtin_amdgcn_readlane(hw, 7);
          const int hwmN = __builtin_amdgcn_readlane(hw, 20), perrC = __builtin_amdgcn_readlane(hw, 30);
          int guard = 0, vd = 0;
          while (((vd = __hip_atomic_load(&S.verdict, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) >> 2) < t) {
            __builtin_amdgcn_s_sleep(SW_SLEEP);
            if (++guard > (1 << 21) || (((guard & 1023) == 0) && __hip_atomic_load(&F.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))) { if (!F.abort) F.abort = __LINE__; break; }
          }
          if ((vd >> 2) == t && (vd & 3) == 1 + candIdx) {
            int needNext = pHwm > hwmN ? pHwm : hwmN;
            if (ahead) { spin_counter(&F.staged, t + 1, &F.abort); const int hwmNN = S4B_UNI(L.stage[tnn % SW_STAGES].sc[TI_HWM]); if (hwmNN + 2 > needNext) needNext = hwmNN + 2; }
            const int big = step_fits_wave(needNext, NBX * (pNbA + pNbB), nc) ? 0 : 1;
            if (lane == 0) { F.root = pNode; F.nb = pNbA + pNbB; F.needBig = big; F.sset = 1 + sw_slot(tn, candIdx); F.selSlot[tn & 1] = candIdx;
                             F.paType = pType; F.paStatus = pStatus; F.paNbA = pNbA; }
            if (ctl && perrC != 0 && lane == 0) *a.errFlag |= S4B_ERR_NODE_CAPACITY;
            if (lane == 0) __hip_atomic_store(&F.paGo, t + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            SW_A(52);
          }
        }
      }
      // (whoever leaves the loop lets nobody wait for an image that is never drawn)
      auto release = [&]() {
        if (lane == 0) {
          if (candIdx == 0) { __hip_atomic_store(&F.rng0Copied, T + 2, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); __hip_atomic_store(&F.img0Ready, T + 2, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                              __hip_atomic_store(&F.pre0Copied, T + 2, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                              F.aheadId[0] = 0; F.aheadId[1] = 0; F.aheadId[2] = 0; __hip_atomic_store(&F.pre0Ready, T + 2, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }
          else { __hip_atomic_store(&F.rng1Copied, T + 2, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); __hip_atomic_store(&F.img1Ready, T + 2, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }
        }
      };
      if (__hip_atomic_load(&F.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) { release(); break; }
      // ---- the proposal of tree tn is settled (by this wave, its sibling or wave 0)
      if (!spin_counter(&F.paGo, t + 1, &F.abort)) { release(); break; }
      if (candIdx == 0) { SW_ABS(7); }
      if (__builtin_amdgcn_readfirstlane(F.needBig)) { bailStep = t; release(); break; }
      if (!ahead) { release(); break; }
      // draws the image of tree `dst` that belongs to this wave from the image (srcTree, srcC): the generator that image left behind,
      // advanced by the draws decide(srcTree) consumes under this wave's hypothesis — one uniform for the accept test of a pending move
      // plus two per leaf of the tree it ends with (leaf count of the source proposal: pNbA; type / status: pType / pStatus)
      auto draw = [&](int srcTree, int srcC, int pType, int pStatus, int pNbA, int dst, bool aheadDraw) {
        const int slot = 1 + candIdx;
        const MTState* src = cand_lds(L.img, srcTree, srcC).rng;
#pragma unroll
        for (int j = 0; j < MTJ; ++j) { const int i = lane + j * 64; if (i < MTW) ((uint32_t*)&F.rngB[candIdx])[i] = ((const uint32_t*)src)[i]; }
        if (lane == 0) {
          if (aheadDraw) __hip_atomic_store(&F.pre0Copied, srcTree, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
          else __hip_atomic_store(candIdx == 0 ? &F.rng0Copied : &F.rng1Copied, srcTree, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        const int drawsAccept = pStatus == 1 ? 1 : 0;
        const int nlNow = pNbA;
        const int nlAcc = pType == MOVE_BIRTH ? nlNow + 1 : (pType == MOVE_DEATH ? nlNow - 1 : nlNow);
        const int hyp0 = drawsAccept + 2 * nlNow, hyp1 = drawsAccept + 2 * nlAcc;
        const bool exists = candIdx == 0 || (drawsAccept == 1 && hyp1 != hyp0);
        const CandSet cdOut = cand_lds(L.img, dst, candIdx);
        if (!exists) { if (lane == 0) cdOut.meta[0] = 0; return; }
        const int hyp = candIdx == 0 ? hyp0 : hyp1;
        WaveModelT<SPL> m;
        static_cast<ModelView&>(m) = a.model;
        m.scratch = S.scratch[slot];
        m.pg.load(M.pg[lane]); m.lpg.load(M.lpg[lane]); m.l1pg.load(M.l1pg[lane]); m.li0.load(M.li0[lane]); m.li1.load(M.li1[lane]);
        m.nc0 = M.nc0[lane]; m.nc1 = M.nc1[lane];
      if constexpr (SPL) m.spTab = spTab;
        spin_counter(&F.staged, dst, &F.abort);
        const TreeStage* st = L.stage + (dst % SW_STAGES);
        const bool laneIn = lane < nc;
        WaveTree curN; WaveCache caN; WaveTables tbN; WaveArrD muN; int cntN;
        curN.nc = nc < 64 ? nc : 64;
        curN.var.r = laneIn ? (int)st->row[TF_VAR][lane] : (int)NODE_FREE; curN.cut.r = (int)(uint16_t)st->row[TF_CUT][lane]; curN.left.r = st->row[TF_LEFT][lane];
        curN.right.r = st->row[TF_RIGHT][lane]; curN.parent.r = st->row[TF_PARENT][lane]; curN.na.r = st->row[TF_NA][lane]; curN.dep.r = st->row[TF_DEP][lane];
        caN.leaf.r = st->row[TF_LEAF][lane]; caN.pre.r = st->row[TF_PRE][lane]; caN.post.r = st->row[TF_POST][lane];
        muN.load(st->mu[lane]); cntN = st->cnt[lane];
        caN.nl = S4B_UNI(st->sc[TI_NL]); caN.ni = S4B_UNI(st->sc[TI_NI]); caN.g = S4B_UNI(st->sc[TI_G]); caN.gn = S4B_UNI(st->sc[TI_GN]); caN.valid = S4B_UNI(st->sc[TI_VALID]);
        caN.logPi = S4B_UNI(st->logPi);
        const int hwmP = S4B_UNI(st->sc[TI_HWM]);
        if (!caN.valid) tv_rebuild_cache(curN, m, caN);
        WaveRng rng; rng.open(&F.rngB[candIdx]);
        rng_advance(&rng, hyp);
        rng.count = 0;
        tbN.prop = curN;
        tbN.binA.r = -1; tbN.binB.r = -1; tbN.insub.r = 0; tbN.list.r = 0;
        Proposal prN;
#ifdef S4B_SWEEP_TIMING
        const long long tPr0 = wall_clock64();
#endif
        const int perr = propose(curN, hwmP, m, &rng, &prN, tbN, caN);
#ifdef S4B_SWEEP_TIMING
        if ((int)SW_BX == SW_TIMED_WG && lane == 0 && wv == 1) { atomicAdd(&g_sw[24 + (prN.type & 3)], (unsigned long long)(wall_clock64() - tPr0)); atomicAdd(&g_sw[36 + (prN.type & 3)], 1ull);
                                                             if (prN.status != 1) atomicAdd(&g_sw[62], 1ull); if (aheadDraw) atomicAdd(&g_sw[69], 1ull); else atomicAdd(&g_sw[64], 1ull); }
#endif
        rng.close();
        // its statistics-half tables -> the table set of the image's slot; the image itself -> the slot
        const int set = 1 + sw_slot(dst, candIdx);
        const int cntOut = prN.hwm;
        if (lane < cntOut) {
          NodeS sN; sN.mu = muN.mine(); sN.binA = (int16_t)tbN.binA.r; sN.binB = (int16_t)tbN.binB.r; sN.insub = (int16_t)tbN.insub.r; sN.pad = 0;
          NodeP pN; pN.var = (int16_t)tbN.prop.var.r; pN.cut = (uint16_t)tbN.prop.cut.r; pN.left = (int16_t)tbN.prop.left.r; pN.right = (int16_t)tbN.prop.right.r;
          L.S[set * SW_NC + lane] = sN; L.SP[set * SW_NC + lane] = pN;
        }
        int16_t* const sO = cdOut.slab;
        wave_tree_store(tbN.prop, sO + SF_VAR * SW_NC, (uint16_t*)(sO + SF_CUT * SW_NC), sO + SF_LEFT * SW_NC, sO + SF_RIGHT * SW_NC, sO + SF_PARENT * SW_NC, cntOut, lane);
        if (lane < cntOut) { sO[SF_BINA * SW_NC + lane] = (int16_t)tbN.binA.r; sO[SF_BINB * SW_NC + lane] = (int16_t)tbN.binB.r; cdOut.insub[lane] = (uint8_t)tbN.insub.r;
                             sO[SF_NA * SW_NC + lane] = (int16_t)tbN.prop.na.r; sO[SF_DEP * SW_NC + lane] = (int16_t)tbN.prop.dep.r; }
        sO[SF_CVAR * SW_NC + lane] = (int16_t)curN.var.r; ((uint16_t*)sO)[SF_CCUT * SW_NC + lane] = (uint16_t)curN.cut.r; sO[SF_CLEFT * SW_NC + lane] = (int16_t)curN.left.r;
        sO[SF_CRIGHT * SW_NC + lane] = (int16_t)curN.right.r; sO[SF_CPARENT * SW_NC + lane] = (int16_t)curN.parent.r; sO[SF_CNA * SW_NC + lane] = (int16_t)curN.na.r;
        sO[SF_CDEP * SW_NC + lane] = (int16_t)curN.dep.r; sO[SF_CLEAF * SW_NC + lane] = (int16_t)caN.leaf.r; sO[SF_CPRE * SW_NC + lane] = (int16_t)caN.pre.r;
        sO[SF_CPOST * SW_NC + lane] = (int16_t)caN.post.r; cdOut.snapMu[lane] = muN.mine(); cdOut.snapCnt[lane] = cntN;
        step_header_store(prN, hwmP, caN.nl, caN.ni, caN.g, caN.gn, caN.logPi, cdOut.head, lane);
#pragma unroll
        for (int j = 0; j < MTJ; ++j) { const int i = lane + j * 64; if (i < MTW) ((uint32_t*)cdOut.rng)[i] = ((const uint32_t*)&F.rngB[candIdx])[i]; }
        if (lane < 4) cdOut.meta[lane] = lane == 0 ? 1 : (lane == 1 ? hyp : (lane == 2 ? perr : drawNo));
      };
      // ---- phase 0: the FINAL image of tree t+1 that belongs to this wave; phase 1 (wave 1 only): image 0 of tree t+2, AHEAD — from image 0
      // of tree t+1 (final since phase 0), assumed to survive decide(tn).  (One loop, one inlined copy of draw(): the kernel sits at its
      // register budget, and a second copy of the drawing code costs seven more spilled registers.)
#pragma unroll 1
      for (int phase = 0; phase < (candIdx == 0 ? 2 : 1); ++phase) {
        int srcTree, srcC, pType, pStatus, pNbA, dst; bool doit;
        if (phase == 0) {
          const int sel = __builtin_amdgcn_readfirstlane(F.selSlot[tn & 1]);
          const int ssetNow = __builtin_amdgcn_readfirstlane(F.sset);
          // drawn ahead from image 0 of tree tn — and image 0 of tree tn (not wave 0's own proposal in its slot) is what survived: it stands
          const bool stands = candIdx == 0 && pre == tnn && sel == 0 && ssetNow != 0;
          srcTree = tn; srcC = sel; dst = tnn; doit = !stands;
          pType = __builtin_amdgcn_readfirstlane(F.paType); pStatus = __builtin_amdgcn_readfirstlane(F.paStatus); pNbA = __builtin_amdgcn_readfirstlane(F.paNbA);
          if (stands && lane == 0) __hip_atomic_store(&F.rng0Copied, tn, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
          srcTree = tnn; srcC = 0; dst = t + 2; doit = false; pType = 0; pStatus = 0; pNbA = 0;
          if (t + 2 < T) {
            // its slot is the one image 0 of tree t-1 lives in: the decider (decide(t-1), its leaf draws from that image's generator) and
            // wave 3 (the early leaf values) are done with it once decDone = t; wave 0's own proposal of this step ended before paGo = t + 1
            spin_counter(&F.decDone, t, &F.abort);
            const CandSet cs1 = cand_lds(L.img, tnn, 0);
            const int hw = lane < 28 ? ((const int32_t*)cs1.head)[lane] : (lane < 31 ? cs1.meta[lane - 28] : 0);
            // (nobody has yet checked that tree t+2 fits the 64 node slots of the wave-register control code — the step that settles tree
            // t+1 does; on a larger tree the walks of propose() over truncated wave arrays need not end: fuzz seed 280 of round 4, again)
            spin_counter(&F.staged, t + 2, &F.abort);
            const bool fits = step_fits_wave(S4B_UNI(L.stage[(t + 2) % SW_STAGES].sc[TI_HWM]) + 2, 0, nc);
            doit = __builtin_amdgcn_readlane(hw, 28) != 0 && fits;
            pType = __builtin_amdgcn_readlane(hw, 0); pStatus = __builtin_amdgcn_readlane(hw, 1); pNbA = __builtin_amdgcn_readlane(hw, 5);
          }
          if (!doit && lane == 0) __hip_atomic_store(&F.pre0Copied, tnn, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (doit && phase == 1) { SW_ABS(5); }
        if (doit) { ++drawNo; draw(srcTree, srcC, pType, pStatus, pNbA, dst, phase == 1); }
        if (doit && phase == 1) { SW_ABS(6); }
        if (phase == 0) { if (lane == 0) __hip_atomic_store(candIdx == 0 ? &F.img0Ready : &F.img1Ready, tnn, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }
        else {
          if (doit) pre = t + 2;
          // (the pass waves route tree t+2 under this image and gather its statistics AHEAD, during step t+1: see LINEARITY)
          if (lane == 0) {
            const CandSet ca = cand_lds(L.img, t + 2, 0);
            const bool there = doit && ca.meta[0] != 0;
            F.aheadId[(t + 2) % 3] = there ? drawNo : 0; F.aheadNb[(t + 2) % 3] = there ? ca.head->pr.nbA + ca.head->pr.nbB : 0;
            __hip_atomic_store(&F.pre0Ready, t + 2, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
          }
        }
      }
      if (wv == 1) { SW_MARK(); }
    }
  } else if (wv == 3) {
    // ====================================================================================== wave 3: the exchange
    int nbPrev = 0;          // bins of the statistics published in the previous step (what this step's gather polls)
    bool prevAlt = false;    // ... which are in the second ring: the previous step speculated and the verdict did not bear it out
    int nSpecSteps = 0, nSpecOk = 0;   // (control workgroup) steps of this launch whose statistics went out before their verdict / were borne out by it: status words 13, 14
    bool prevOk = false;     // the previous step published before its verdict and the verdict bore it out (linear statistics: its ahead pass ran beside that verdict)
    bool prevSelf = false;   // ... and it was THIS wave that published (linear statistics): nobody sets F.published for that step
    for (int t = 0; t <= T; ++t) {
      const bool doDecide = t > 0, doPropose = t < T;
      int specNb = 0;
      SW_KERNARGS();
      // ---- wave 3: totals of statistics(t-1) from the exchange words, 2 nb words x XC_COPIES copies
      // (polling starts when this workgroup's own partials are out: polls sent earlier only queue in front of the pass waves' loads; ONE poll in
      // flight: a second one issued before the first is back — round 5 — makes the sweep 12 % slower, the polls crowd the arriving atomics)
      // ---- while nothing can arrive yet: everything of the leaf draws of tree t-1 in case its pending move is not accepted (below) that does
      // not wait for the statistics.  The standard normal deviates depend on the generator words alone (which words a leaf takes depends on the
      // statistics only through "every leaf holds observations"); the observation COUNT of a leaf is the one the tree carries since its last
      // update (the tree has not changed, the data do not), hence the posterior precision and standard deviation; both assumptions are checked
      // when the totals are in (else: the whole arithmetic then, as before).  Likewise whether this step speculates (see below).
      // (The surviving proposal of tree t-1 and its generator are final since paGo = t, which this wave has seen; the decider touches the
      // generator only after the totals; image 0 of tree t is out since the previous step and stays until this step's verdict.)
      double zPre = 0.0, ppPre = 0.0, denPre = 1.0, sdPre = 0.0, wPre = 0.0, muOldPre = 0.0; bool preOk = false; int preNl = 0, preN = 0, preBA = 0, preMti0 = 0, specNbPre = 0, seqImg = 0;
      if (doDecide) {
        const CandSet cs = cand_lds(L.img, t - 1, __builtin_amdgcn_readfirstlane(F.selSlot[(t - 1) & 1]));
        const int32_t* const hd = (const int32_t*)cs.head;
        preNl = S4B_UNI(hd[21]);
        preMti0 = S4B_UNI((int)cs.rng->mti) + (S4B_UNI(hd[1]) == 1 ? 1 : 0);
        preOk = preMti0 + 2 * preNl <= 624;
        const bool in = lane < preNl;
        preN = in ? (int)cs.slab[SF_CLEAF * SW_NC + lane] & 63 : 0;
        preBA = (int)cs.slab[SF_BINA * SW_NC + preN] & 63;
        muOldPre = cs.snapMu[preN];
        wPre = in ? (double)cs.snapCnt[preN] : 0.0;
        const int k = (preOk && in) ? preMti0 + 2 * lane : 0;
        zPre = leaf_deviate(mt_word_to_unif(cs.rng->mt[k]), mt_word_to_unif(cs.rng->mt[k + 1]));
        ppPre = wPre / (M.sigma * M.sigma); denPre = a.model.leafPrec + ppPre; sdPre = 1.0 / sqrt(denPre);
        // (pinned here: the optimiser otherwise sinks all of this arithmetic into the branch that uses it — behind the totals)
        asm volatile("" : "+v"(zPre), "+v"(ppPre), "+v"(denPre), "+v"(sdPre), "+v"(muOldPre), "+v"(wPre));
        asm volatile("" : "+v"(preN), "+v"(preBA));
        if (!STREAM && doPropose && !solo) {      // (a one-workgroup launch does not speculate — it could, its reducing lanes holding the sums until the verdict: BASELINE config 4 984 - 994 it/s with, 1 016 - 1 024 without: the accumulation then runs beside the decider on the same SIMD)
          spin_counter(&F.img0Ready, t, &F.abort);
          const CandSet c0 = cand_lds(L.img, t, 0);
          const int nbImg = S4B_UNI(c0.head->pr.nbA) + S4B_UNI(c0.head->pr.nbB);
          if (S4B_UNI(c0.meta[0]) != 0 && nbImg >= 1 && nbImg <= 8) { specNbPre = nbImg; seqImg = S4B_UNI(c0.meta[3]); }
        }
      }
      // (this workgroup's own partials of statistics(t-1) are out: published by the pass waves — or, linear statistics, by this wave itself in the step before)
      if (doDecide && hasObs && !(S4B_LINEAR && prevSelf && !prevAlt)) spin_counter(prevAlt ? &F.publishedAlt : &F.published, t, &F.abort);
      if (doDecide) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the clearing stores of the previous step are out: before this step's specReady, hence before this workgroup publishes again
        unsigned long long* const xPrev = x.xbuf + (size_t)((prevAlt ? XC_RING : 0) + ((t + XC_RING - 1) & (XC_RING - 1))) * XC_BUF_WORDS;
        const int nw = solo ? 0 : 2 * NBX * nbPrev;       // (solo: wave 4 has written the totals themselves)
        bool fine = true;
        // (the first poll waits ~1.1 us: this workgroup has just published, the last of the others is 1 - 2.5 us behind the first, and every
        // poll of the 256 workgroups is eight more requests to the cache lines the arriving atomics need — round 5: 467 -> 488 iterations/s)
        if (nw > 0 && !STREAM) __builtin_amdgcn_s_sleep(S4B_POLL_DELAY);
        for (int half = 0; half * 64 < nw; ++half) {
          const int wi = half * 64 + lane;
          const bool in = wi < nw;
          unsigned long long w[XC_COPIES];
          bool done = false;
          for (int g = 0; g < (1 << 20) && !done; ++g) {
            bool ok = true;
#pragma unroll
            for (int c = 0; c < XC_COPIES; ++c) w[c] = in ? xc_load(xPrev + (size_t)c * XC_WORDS + wi) : 0ull;
#pragma unroll
            for (int c = 0; c < XC_COPIES; ++c) {
              const unsigned want = c <= NP ? (unsigned)((NP - c) / XC_COPIES + 1) : 0u;   // workgroups b (the control workgroup too) with b % XC_COPIES == c
              ok = ok && (!in || (unsigned)(w[c] >> 58) == want);
            }
            done = __all(ok);
            if (!done) { __builtin_amdgcn_s_sleep(STREAM ? 8 : S4B_POLL_SLEEP); if ((g & 1023) == 1023 && __hip_atomic_load(&F.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break; }
          }
          fine = fine && done;
          unsigned long long f0 = 0ull, f1 = 0ull, fc = 0ull;
#pragma unroll
          for (int c = 0; c < XC_COPIES; ++c) { f0 += w[c] & ((1ull << 58) - 1); f1 += w[c] & ((1ull << 37) - 1); fc += (w[c] >> 37) & ((1ull << 21) - 1); }
          // even lanes hold word 0 of their bin, odd lanes word 1: bring both to the even lane
          const unsigned long long g1 = __shfl_down(f1, 1), gc = __shfl_down(fc, 1);
          if (in && (lane & 1) == 0) {
            const long long H = (long long)(f0 - ((unsigned long long)(NP + 1) << 52)), Lo = (long long)(g1 - ((unsigned long long)(NP + 1) << 31));
            const int k = wi >> 1;
            const double tot = (double)H * (1.0 / 16777216.0) + (double)Lo * (1.0 / 36028797018963968.0);
            F.totS[k] = WT ? tot * x.wUnscale : tot;
            F.totC[k] = (double)(long long)gc;
          }
        }
        if (!fine && lane == 0) { F.abort = __LINE__; *a.errFlag |= S4B_ERR_INTERNAL | S4B_ERR_I_GATHER; }
#ifdef S4B_SWEEP_WG
        if (lane == 0) {
          const unsigned long long nw = (unsigned long long)wall_clock64();
          const int b = (int)SW_BX;
          F.t0[t & 3] = (long long)nw;
          if (t > 0 && t < T && b < 256) { atomicAdd(&g_wg[b * 16 + 2], nw); atomicAdd(&g_wg[b * 16 + 3], 1ull); }
          if (t > 1 && t < T && b < 256) {
            const unsigned long long mxp = atomicAdd(&g_pubMax[(t - 1) & 7], 0ull), mnp = atomicAdd(&g_pubMin[(t - 1) & 7], 0ull);
            if (mxp != 0ull && mnp != ~0ull && mnp != 0ull && nw - mxp < 10000ull && mxp - mnp < 10000ull) { atomicAdd(&g_wg[b * 16 + 4], nw - mxp); atomicAdd(&g_wg[b * 16 + 5], 1ull); atomicAdd(&g_wg[b * 16 + 6], mxp - mnp); }
            if (b == 0) { atomicExch(&g_pubMax[(t + 3) & 7], 0ull); atomicExch(&g_pubMin[(t + 3) & 7], ~0ull); }
          }
        }
#endif
#ifdef S4B_SWEEP_TIMING
        SW_AP(40);
#endif
        if (lane == 0) __hip_atomic_store(&S.arrived, t, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        SW_T(1);
        // ---- the leaf values of tree t-1 in case its pending move is not accepted (see wave 0): lane i owns leaf i of the DFS list
        {
          const int nl = preNl, n = preN;
          const bool in = lane < nl;
          const double lc = F.totC[preBA], ls = F.totS[preBA];
          const double lw = WT ? F.totS[nbPrev + preBA] : lc;
          const bool ne = in && lc != 0.0;
          const unsigned long long mask = __ballot(ne);
          const int cntNe = __popcll(mask);
          const bool valid = preMti0 + 2 * cntNe <= 624;        // (else the block of generator words is renewed among these draws: wave 0 does it)
          double v = 0.0;
          if (!WT && preOk && cntNe == nl && __all(!in || lc == wPre)) {     // every leaf took the words assumed above and holds the observations it held
            if (ne) v = leaf_value_parts(ppPre, denPre, sdPre, lc, ls, zPre);
          } else {
            const CandSet cs = cand_lds(L.img, t - 1, __builtin_amdgcn_readfirstlane(F.selSlot[(t - 1) & 1]));
            const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
            const int k = (ne && valid) ? preMti0 + 2 * rank : 0;
            const uint32_t y1 = cs.rng->mt[k], y2 = cs.rng->mt[k + 1];
            if (ne) v = leaf_value(lw, ls, mt_word_to_unif(y1), mt_word_to_unif(y2), M.sigma * M.sigma, a.model.leafPrec);
          }
          // (old and new value of the leaf as one record: the pass waves may fold them SPECULATIVELY before the decider has written
          // anything — see the pass waves; the decider writes the same old values at its verdict)
          // (linear statistics: the pass waves read the table of step t-2 — same parity — beside that step's verdict and when they fold; this wave's
          // own publishing no longer waits for them to be through with a step)
          if (S4B_LINEAR && !STREAM) spin_counter(&F.passSeen, 4 * (t - 1), &F.abort);
          if (in && valid) { NodeA na; na.muOld = muOldPre; na.muNew = v; (L.A + (STREAM ? 0 : (t & 1)) * SW_NC)[n] = na; }
          if (S4B_LINEAR && !STREAM && in && valid) L.dtab[(t & 1) * SW_NC + n] = muOldPre - v;
          // SPECULATION (see the pass waves): "the pending move of tree t-1 is not accepted and image 0 of tree t is its proposal" — everything
          // that outcome needs is here now: the pass waves publish the statistics of tree t under it without waiting for the verdict.  Whether
          // a step speculates is a function of the chain alone (every workgroup arrives at the same answer, the control workgroup included).
#if S4B_LINEAR
          // LINEARITY (round 6).  The statistics of tree t were gathered one step AHEAD by the pass waves — bin sums of the partial residual with tree t-1
          // still missing (preS / preC) and, per bin, how many of its observations sit in which leaf of tree t-1 (ctab) —, under the image of tree t's
          // proposal that carries drawing number preSeq.  If that is the image that stands now, the new leaf values above complete them: per bin
          // sum + SUM over the leaves of tree t-1 of count x (old value - new value) — leaves x bins multiply-adds instead of a pass over the
          // observations — and THIS wave publishes, 1.5 us after the totals instead of 4.  Whether a step does so is a function of the chain alone.
          // (the decider waits for specReady — wave 3's leaf values are in the table —, not for what follows)
          if (lane == 0) { F.specCnt = cntNe; __hip_atomic_store(&F.specReady, (t << 1) | (valid ? 1 : 0), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }
          int nbLin = 0; bool dirty = false;
          if (specNbPre) {
            // the ahead pass of the step before is through — A: it ran beside that step's verdict, which then bore the step out; B: the step was redone the
            // old way and the pass followed it
#ifdef S4B_SWEEP_WGD
            const long long tW0 = wall_clock64();
#endif
            if (prevOk) spin_counter(&F.preDoneA, t, &F.abort); else spin_counter(&F.preDoneB, t, &F.abort);
#ifdef S4B_SWEEP_WGD
            if (lane == 0 && t > 1 && t + 1 < T && (int)SW_BX < 256) sw_dur_add((int)SW_BX * 64 + 7, (unsigned long long)(wall_clock64() - tW0));
#endif
            const int pnb = S4B_UNI(F.preNb[t & 1]), pseq = S4B_UNI(F.preSeq[t & 1]);
            if (pnb == specNbPre && pseq == seqImg) nbLin = pnb;
            dirty = pnb != 0;
          }
          specNb = valid ? nbLin : 0;
          if (lane == 0) { F.specNb[t & 1] = specNb; __hip_atomic_store(&F.linReady, t, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }
          SW_A(51); if (specNb) SW_W(8);
          if (specNb) {
            unsigned long long* const ring = x.xbuf + (size_t)(t & (XC_RING - 1)) * XC_BUF_WORDS;
            // (the control workgroup owns no observations, but it ARRIVES at every exchange — see below)
            if (ctl) { if (lane < specNb) xc_publish(ring, lane, 0.0, 0, a.errFlag); }
            else {
              const unsigned* const ct = L.ctab + (size_t)(t & 1) * SW_CT_WORDS;
              double sL = 0.0; unsigned cL = 0u;      // (the count of a bin: every one of its observations sits in exactly one leaf of the tree before)
              if (lane < specNb) {
                const double* const ps = L.preS + (t & 1) * SW_PW * 8 + lane;
                sL = ((ps[0] + ps[8]) + ps[16]) + ps[24];      // (the pass waves' pre-sums, in the order of the waves)
              }
              const int bIdx = lane & 7;
              const double dl = (in && valid) ? muOldPre - v : 0.0;      // lane i: leaf i of the tree (a leaf without observations has no counts)
              const int dlo = __double2loint(dl), dhi = __double2hiint(dl);
              for (int i0 = 0; i0 < nl; i0 += 4) {      // (lanes beyond the leaves carry a zero difference: the tail of a group of four adds nothing)
                uint4 c4[4]; double di[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                  const int i = i0 + u;      // (< 64: a tree of the wave path has at most 32 leaves)
                  const int nd = __builtin_amdgcn_readlane(n, i) & (SW_NC - 1);
                  di[u] = __hiloint2double(__builtin_amdgcn_readlane(dhi, i), __builtin_amdgcn_readlane(dlo, i));
                  c4[u] = *reinterpret_cast<const uint4*>(ct + (size_t)(nd * 8 + bIdx) * SW_CC);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                  const unsigned cu = (i0 + u < nl) ? c4[u].x + c4[u].y + c4[u].z + c4[u].w : 0u;      // (the tail of a group of four reads the row of node 0 again)
                  cL += cu; sL = fma((double)cu, di[u], sL);
                }
              }
              if (lane < specNb) xc_publish(ring, lane, sL, (int)cL, a.errFlag);
#ifdef S4B_SWEEP_WG
              if (lane == 0 && t > 0 && t < T && (int)SW_BX < 256) {
                const unsigned long long nw = (unsigned long long)wall_clock64();
                atomicAdd(&g_wg[SW_BX * 16], nw - (unsigned long long)F.t0[t & 3]); atomicAdd(&g_wg[SW_BX * 16 + 1], 1ull);
                atomicMax(&g_pubMax[t & 7], nw); atomicMin(&g_pubMin[t & 7], nw);
              }
#endif
            }
          }
          // the counts of this parity go back to zero for the pass after next (nobody adds to them before this step's specReady has been seen)
          if (dirty) {
            uint4* const z = reinterpret_cast<uint4*>(L.ctab + (size_t)(t & 1) * SW_CT_WORDS);
            const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
            for (int i = lane; i < SW_CT_WORDS / 4; i += 64) z[i] = zero;
          }
#else
          specNb = valid ? specNbPre : 0;
          if (lane == 0) { F.specCnt = cntNe; F.specNb[t & 1] = specNb; __hip_atomic_store(&F.specReady, (t << 1) | (valid ? 1 : 0), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }
          SW_A(51); if (specNb) SW_W(8);
          // (the control workgroup owns no observations, but it ARRIVES at every exchange — see below)
          if (ctl && !solo && specNb && lane < NBX * specNb) xc_publish(x.xbuf + (size_t)(t & (XC_RING - 1)) * XC_BUF_WORDS, lane, 0.0, 0, a.errFlag);
#endif
        }
        // re-arm: the exchange buffers of step t-2 — the ones step t+2 publishes into — are dead: whoever has published in step t-1, and
        // everybody has (the totals of this step are complete), had gathered them before.  (Completion: see the top of the next step.)
        if (!ctl && !solo) {
          for (int c = (int)SW_BX; c < 2 * XC_COPIES; c += NP) {   // (pass workgroup b re-arms copies b, b + NP, ... of the two rings)
            unsigned long long* z = x.xbuf + (size_t)((c >= XC_COPIES ? XC_RING : 0) + ((t + 2) & (XC_RING - 1))) * XC_BUF_WORDS + (size_t)(c & (XC_COPIES - 1)) * XC_WORDS;
            __hip_atomic_store(z + lane, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(z + 64 + lane, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
      }
      if (__hip_atomic_load(&F.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
      if (!doPropose) break;
      if (!spin_counter(&F.paGo, t + 1, &F.abort)) break;
      SW_G(94);
      const int nb = __builtin_amdgcn_readfirstlane(F.nb);
      // was the speculation of this step borne out?  (the pass waves apply the same test)
      const bool specOk = specNb != 0 && sweep_spec_confirmed(F, t, specNb);
      prevAlt = specNb != 0 && !specOk;
      prevOk = specOk; prevSelf = specNb != 0;
      nSpecSteps += specNb != 0 ? 1 : 0; nSpecOk += specOk ? 1 : 0;
      if (ctl && !solo && lane < NBX * nb && !specOk) {
        // The control workgroup owns no observations, but it ARRIVES at every exchange (a zero contribution): nobody can finish
        // gathering exchange t before this workgroup has gathered exchange t-1, so no pass workgroup ever runs more than one step
        // ahead of it — and re-arms a buffer of the ring that this workgroup has still to read.
        xc_publish(x.xbuf + (size_t)((prevAlt ? XC_RING : 0) + (t & (XC_RING - 1))) * XC_BUF_WORDS, lane, 0.0, 0, a.errFlag);
      }
      nbPrev = nb;
      SW_MARK();
      if (__builtin_amdgcn_readfirstlane(F.needBig)) { bailStep = t; break; }
    }
    if (ctl && lane == 0) { SW_KERNARGS(); x.status[13] = nSpecSteps; x.status[14] = nSpecOk; }     // (host-mapped words, once per launch: s4b_get_sweep_spec)
  } else {
    // ====================================================================================== waves 4-7: the pass waves
    const int pw = wv - 4, pt = pw * 64 + lane;       // pass wave / pass thread of the workgroup
    const int64_t stride = (int64_t)NP * SW_PT;
    const int64_t q0 = (int64_t)SW_BX * SW_PT + pt;
    PassBar bar; bar.ctr = &F.bar; bar.abortFlag = &F.abort; bar.epoch = 0; bar.tacc = F.tacc; bar.totS = F.totS; bar.totC = F.totC; bar.solo = solo; bar.arr = &F.statArr;
    if constexpr (STREAM) {
      // ---- streaming pass (see stream_pass): per step, wait for the verdict, the leaf values and the settled proposal, then one pass over
      // the thread's quads — finish tree t-1, count tree t —, one block reduction per eight bins, publish
      for (int t = 0; t <= T; ++t) {
        const bool doDecide = t > 0, doPropose = t < T;
        const int tn = doPropose ? t : 0;
        SW_KERNARGS();
        const int64_t nQuads = (a.n + 3) >> 2;
        if (pw == 0 && doPropose) {      // trees are staged two steps before they are decided (the image waves draw one step ahead)
          if (t == 0 && T > 1) stage_tree(a, L.stage, 1, lane);
          // (its stage is the one of tree t-1: wave 2 may still be drawing image 1 of that tree from it — since round 6 the verdict no longer waits for an image 1 it does not need)
        if (t + 2 < T) { if (t >= 1) spin_counter(&F.img1Ready, t - 1, &F.abort); stage_tree(a, L.stage, t + 2, lane); }
          if (lane == 0) __hip_atomic_store(&F.staged, t + 2 < T ? t + 2 : T - 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (doDecide) { spin_counter(&F.foldReady, t, &F.abort); spin_counter(&F.tablesReady, t, &F.abort); }
        if (doPropose) spin_counter(&F.paGo, t + 1, &F.abort);
        if (__hip_atomic_load(&F.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
        StreamStep st;
        st.root = __builtin_amdgcn_readfirstlane(F.root); st.sset = doPropose ? __builtin_amdgcn_readfirstlane(F.sset) : 0; st.base = 0;
        st.prevAcc = doDecide ? __builtin_amdgcn_readfirstlane(F.prevAcc) : 0; st.prevRoot = __builtin_amdgcn_readfirstlane(F.prevRoot);
        st.prevDeath = __builtin_amdgcn_readfirstlane(F.prevDeath);
        const int nb = doPropose ? __builtin_amdgcn_readfirstlane(F.nb) : 0;
        const bool bail = doPropose && __builtin_amdgcn_readfirstlane(F.needBig) != 0;
        if (hasObs) {
          unsigned long long* const xCur = x.xbuf + (size_t)(t & (XC_RING - 1)) * XC_BUF_WORDS;
          double* const partOut = a.partF + (size_t)(t & 1) * 3 * a.binCap * a.gridF;
          const int tA = doDecide ? t - 1 : 0;
          if (!doPropose) stream_pass<4, true, false>(a, L, bar, st, tn, tA, q0, stride, nQuads, xCur, partOut, false, pw, lane);
          else {
            for (int base = 0; base < nb; base += 8) {     // (eight bins per pass over the observations; the first pass also finishes tree t-1)
              if (base > 0) pass_barrier(bar);
              st.base = base;
              const int nbThis = nb - base < 8 ? nb - base : 8;
              if (doDecide && base == 0) stream_pass_n<true, true>(nbThis, a, L, bar, st, tn, tA, q0, stride, nQuads, xCur, partOut, bail, pw, lane);
              else stream_pass_n<false, true>(nbThis, a, L, bar, st, tn, tA, q0, stride, nQuads, xCur, partOut, bail, pw, lane);
            }
          }
          if (pw == 0 && lane == 0 && doPropose) __hip_atomic_store(&F.published, t + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (bail) { bailStep = t; break; }
      }
    } else {
#if S4B_LINEAR
    // LINEARITY (round 6; VERDICT r05 item 1).  Until round 5 the chain of a step was  totals(t-1) -> leaf values of tree t-1 -> O(N) statistics of tree t
    // (residual with tree t-1 folded in on the fly) -> publish -> exchange.  The bin sums are LINEAR in the leaf values of tree t-1:
    //     sum over bin b of tree t of (R_{t-1} + fit_t)  =  sum over bin b of (R_{t-2} + fit_t)  +  SUM over leaves l of tree t-1 of C[l][b] (old - new value)(l)
    // with C[l][b] = how many observations of bin b sit in leaf l of tree t-1 — an INTEGER that depends on nothing the totals produce.  So the pass
    // waves run the O(N) pass for tree t+1 one step AHEAD, while the exchange of tree t travels and wave 0 decides: residual as it stands in the
    // registers (trees <= t-2) + tree t-1 folded in on the fly (wave 3's early values, as the speculative pass of round 5 did) -> pre-sums preS / preC
    // of tree t+1's bins under image 0 of its proposal, which wave 1 draws two steps ahead, + the contingency counts against the leaves of tree t
    // (ctab, LDS atomics).  When the totals of tree t are in, wave 3 has its new leaf values 1.2 us later, completes the workgroup's statistics of tree
    // t+1 with (leaves x bins) multiply-adds and publishes them itself: no observation is touched between the totals and the publish.
    // State of a pass thread at the top of step t: r = residual with trees <= t-2 folded in; lfPrev / bbPrev = leaf ids / B bins of tree t-1 (relabelling under
    // an accepted move); lfCur / bbCur = leaf ids of tree t and its B bins under the image with drawing number idCur (0: not routed).
    // A step whose verdict does not bear the assumptions out (the move of tree t-1 accepted, another image of tree t) is redone the old way — fold,
    // route, statistics, second ring — and the ahead pass for tree t+1 FOLLOWS it (zero leaf-value table: the residual then holds tree t-1 already).
    SweepObs O;
    lfq_t lfCur[SW_PF]; unsigned bbCur[SW_PF]; int idCur = 0;
    lfq_t lfNext[SW_PF];      // leaf ids of tree t+1, requested a whole step before they are used (the request of a step's own leaf ids cost every step 2.4 us of memory latency)
    {
      SW_KERNARGS();
      const int64_t nQuads = (a.n + 3) >> 2;
#pragma unroll
      for (int j = 0; j < SW_PF; ++j) {
        const int64_t qd = q0 + (int64_t)j * stride;
        double2 r01 = make_double2(0.0, 0.0), r23 = make_double2(0.0, 0.0);
        lfCur[j] = 0u; bbCur[j] = 0xffffffffu; lfNext[j] = 0u;
        if (hasObs && qd < nQuads) { const int64_t i0 = qd << 2; r01 = *reinterpret_cast<const double2*>(a.R + i0); r23 = *reinterpret_cast<const double2*>(a.R + i0 + 2);
                                     lfCur[j] = lfq_pack(__builtin_nontemporal_load(reinterpret_cast<const us4_t*>(a.leaf + i0)));
                                     if (T > 1) lfNext[j] = lfq_pack(__builtin_nontemporal_load(reinterpret_cast<const us4_t*>(a.leaf + (size_t)a.npad + i0))); }
        O.r[j][0] = r01.x; O.r[j][1] = r01.y; O.r[j][2] = r23.x; O.r[j][3] = r23.y;
        O.lfPrev[j] = 0u; O.bbPrev[j] = 0xffffffffu;
      }
    }
    const int64_t q0w = q0;
    SW_DDECL();
    for (int t = 0; t <= T; ++t) {
      const bool doDecide = t > 0, doPropose = t < T;
      const bool spec = doDecide && doPropose;
      const bool haveNext = t + 1 < T;
      SW_KERNARGS();
      const int64_t nQuads = (a.n + 3) >> 2;
      // (the thread's first quad, opaque once per step: the sixteen 64-bit observation indices derived from it are otherwise kept across the
      // steps — 32 registers the residual and the statistics need, i.e. spills)
      int64_t q0 = q0w;
      asm volatile("" : "+v"(q0));
      // quads the threads of this workgroup own at most (thread 0 owns the most): a launch over few observations skips the unrolled work of the others
      int jMax = 0;
#pragma unroll
      for (int j = 0; j < SW_PF; ++j) jMax += ((int64_t)SW_BX * SW_PT + (int64_t)j * stride < nQuads) ? 1 : 0;
      jMax = __builtin_amdgcn_readfirstlane(jMax);
      // ---- leaf ids of the tree AFTER next: requested now, used from the next step on (lfNext — the tree whose statistics are gathered ahead during this step — was
      // requested a step ago)
      // (issued behind the routing of this step, whose column loads would otherwise wait for them: the memory counter retires in order)
      // (kept as loaded — 16-bit ids — until the end of the step: packing them is their first use, and the wait for the memory counter sits in front of the first use)
      us4_t lfAfter[SW_PF]; unsigned bbNext[SW_PF]; int idNext = 0, nbNext = 0;
#pragma unroll
      for (int j = 0; j < SW_PF; ++j) { lfAfter[j].x = 0; lfAfter[j].y = 0; lfAfter[j].z = 0; lfAfter[j].w = 0; bbNext[j] = 0xffffffffu; }
      // ---- wave 4: tree t+2, main arrays -> stage (the image waves propose for it during this step)
      if (pw == 0 && doPropose) {      // trees are staged two steps before they are decided (the image waves draw one step ahead)
        if (t == 0 && T > 1) stage_tree(a, L.stage, 1, lane);
        // (its stage is the one of tree t-1: wave 2 may still be drawing image 1 of that tree from it — since round 6 the verdict no longer waits for an image 1 it does not need)
        if (t + 2 < T) { if (t >= 1) spin_counter(&F.img1Ready, t - 1, &F.abort); stage_tree(a, L.stage, t + 2, lane); }
        if (lane == 0) __hip_atomic_store(&F.staged, t + 2 < T ? t + 2 : T - 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      const NodeA* const At = L.A + (t & 1) * SW_NC;      // leaf-value table of this step
      int nbSpec = 0;
      bool bailNow = false, quit = false;
      bool ranAhead = false;       // an ahead pass of this step has counted into the tables of tree t+1
      // ---- two places run the ahead pass for tree t+1 — beside the verdict of a step wave 3 has published (phase 0), behind a step done the old way
      // (phase 1) — through ONE inlined copy of the pass (the kernel sits at its register and instruction-cache budget)
#pragma unroll 1
      for (int phase = 0; phase < 2; ++phase) {
        // (opaque once per phase: what is derived from the thread's first quad and from its lane id — sixteen 64-bit observation indices, LDS addresses of its
        // reduction slots and counts — is invariant in this two-trip loop; hoisted out of it, it stays live across both phases and spills)
        int64_t q0p = q0; asm volatile("" : "+v"(q0p));
        int lnP = lane; asm volatile("" : "+v"(lnP));
        // (likewise the packed leaf ids and bins: their sixteen byte fields, and the table addresses formed from them, are invariant in the loop too)
#pragma unroll
        for (int j = 0; j < SW_PF; ++j) asm volatile("" : "+v"(O.lfPrev[j]), "+v"(lfCur[j]), "+v"(lfNext[j]), "+v"(O.bbPrev[j]), "+v"(bbCur[j]));
        bool run = false;
        int routeId = 0;           // != 0: route tree t+1 under image 0 of its proposal as it stands in its slot now (drawing number routeId)
        const double* foldD = L.dtab + (t & 1) * SW_NC;      // (differences old - new value of tree t-1: wave 3's, before specReady)
        if (phase == 0) {
          // ---- image 0 of tree t+1's proposal as wave 1 drew it AHEAD (during the step before this one)
          if (!solo && spec && haveNext) {
            SW_D(0);
            if (!spin_counter(&F.pre0Ready, t + 1, &F.abort)) { quit = true; break; }
            SW_D(1);
            routeId = __builtin_amdgcn_readfirstlane(F.aheadId[(t + 1) % 3]);
            if (routeId != 0) nbNext = __builtin_amdgcn_readfirstlane(F.aheadNb[(t + 1) % 3]);
          }
        } else {
          // ---- the verdict is out: old leaf values, which observations move and where to
          bool bothHalves = false;
          unsigned toP[SW_PF];      // node the observation ends up in (one byte per observation)
#pragma unroll
          for (int j = 0; j < SW_PF; ++j) toP[j] = 0u;
          if (doDecide) {
            spin_counter(&F.foldReady, t, &F.abort);
            bothHalves = __builtin_amdgcn_readfirstlane(F.bothStep) == t;
            if (nbSpec) {
              spin_counter(&F.tablesReady, t, &F.abort);
              spin_counter(&F.paGo, t + 1, &F.abort);
              if (__hip_atomic_load(&F.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) { quit = true; break; }
              if (sweep_spec_confirmed(F, t, nbSpec)) {
                // borne out: fold tree t-1 in — the same two operations in the same order as the pass on the fly — and the step is over
                if (hasObs) {
#pragma unroll
                  for (int j = 0; j < SW_PF; ++j) {
                    const unsigned pl[4] = LFQ4(O.lfPrev[j]);
                    NodeA na[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) na[e] = At[pl[e] & 63u];
#pragma unroll
                    for (int e = 0; e < 4; ++e) { O.r[j][e] += na[e].muOld; O.r[j][e] -= na[e].muNew; }
                  }
                }
                if (pw == 1) { SW_G(93); SW_W(11); }
                SW_D(5);
                break;
              }
              // not borne out: what the ahead pass of this step counted is void — its tables are cleared before anybody counts into them again —, and
              // the reduction slots are free again once every pass wave is here
              if (ranAhead) {
                pass_barrier(bar);      // (the ahead pass has no barrier of its own: every pass wave must be through with its counting before the tables are cleared)
                unsigned* const ct = L.ctab + (size_t)((t + 1) & 1) * SW_CT_WORDS;
                for (int i = pw * 64 + lnP; i < SW_CT_WORDS; i += SW_PT) ct[i] = 0u;
              }
              if (hasObs || ranAhead) pass_barrier(bar);
            }
            if (hasObs && bothHalves) {
              // the move was not accepted and both halves of the leaf-value table came with the verdict: nobody moves, one 16-byte read
              // per observation, the same two operations in the same order as below
#pragma unroll
              for (int j = 0; j < SW_PF; ++j) {
                const unsigned pl[4] = LFQ4(O.lfPrev[j]);
                NodeA na[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) na[e] = At[pl[e] & 63u];
#pragma unroll
                for (int e = 0; e < 4; ++e) { O.r[j][e] += na[e].muOld; O.r[j][e] -= na[e].muNew; }
              }
            } else if (hasObs) {
              const int prevAcc = __builtin_amdgcn_readfirstlane(F.prevAcc), prevRoot = __builtin_amdgcn_readfirstlane(F.prevRoot), prevDeath = __builtin_amdgcn_readfirstlane(F.prevDeath);
              const unsigned accM = sw_mask(prevAcc != 0), deathM = sw_mask(prevDeath != 0);
              uint16_t* const prevPlane = a.leaf + (size_t)(t - 1) * a.npad;
#pragma unroll
              for (int j = 0; j < SW_PF; ++j) {
                const int64_t qd = q0p + (int64_t)j * stride;
                const int valid = qd < nQuads ? ((a.n - (qd << 2)) >= 4 ? 4 : (int)(a.n - (qd << 2))) : 0;
                const unsigned pl[4] = LFQ4(O.lfPrev[j]);
                // every table read unconditional, every index valid either way (leaf ids beyond n are 0: those residuals are never
                // used), results merged with opaque masks: all reads of the thread's 16 observations are in flight together
                double muOld[4]; unsigned ain[4], via[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  muOld[e] = At[pl[e]].muOld; ain[e] = L.Ain[pl[e]];
                  via[e] = L.b2n[(O.bbPrev[j] >> (8 * e)) & 63u];
                }
                unsigned nl[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  const unsigned m = (0u - (unsigned)(ain[e] != 0u)) & accM;
                  nl[e] = sw_sel(m, sw_sel(deathM, (unsigned)prevRoot, via[e]), pl[e]) & 63u;
                  O.r[j][e] += muOld[e];
                }
                toP[j] = nl[0] | (nl[1] << 8) | (nl[2] << 16) | (nl[3] << 24);
                if (prevAcc && valid > 0) { us4_t o4; o4.x = (unsigned short)nl[0]; o4.y = (unsigned short)nl[1]; o4.z = (unsigned short)nl[2]; o4.w = (unsigned short)nl[3];
                                            __builtin_nontemporal_store(o4, reinterpret_cast<us4_t*>(prevPlane + (qd << 2))); }
              }
            }
          }
          // ---- the leaf values of tree t-1 are out and the proposal of tree t is settled
          if (doDecide) spin_counter(&F.tablesReady, t, &F.abort);
          if (doPropose) spin_counter(&F.paGo, t + 1, &F.abort);
          if (__hip_atomic_load(&F.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) { quit = true; break; }
          const int root = __builtin_amdgcn_readfirstlane(F.root), nb = doPropose ? __builtin_amdgcn_readfirstlane(F.nb) : 0, sset = __builtin_amdgcn_readfirstlane(F.sset);
          const bool bail = doPropose && __builtin_amdgcn_readfirstlane(F.needBig) != 0;
          bailNow = bail;
          if (hasObs) {
            // the B bins under the surviving proposal: the ones this thread routed a step ago when that very drawing of image 0 survived, else route now
            unsigned bb[SW_PF];
            const int set0 = 1 + sw_slot(t, 0);
            const bool same = doPropose && sset == set0 && idCur != 0 && S4B_UNI(cand_lds(L.img, t, 0).meta[3]) == idCur;
            if (same) {
#pragma unroll
              for (int j = 0; j < SW_PF; ++j) bb[j] = bbCur[j];
            } else if (doPropose) {
              const NodeS* const Ss[1] = {L.S + sset * SW_NC}; const NodeP* const SPs[1] = {L.SP + sset * SW_NC}; const int roots[1] = {root}; const bool haves[1] = {true};
              unsigned bb1x[1][SW_PF];
              sweep_route<1>(a, Ss, SPs, roots, haves, lfCur, q0p, stride, nQuads, bb1x);
#pragma unroll
              for (int j = 0; j < SW_PF; ++j) bb[j] = bb1x[0][j];
            } else {
#pragma unroll
              for (int j = 0; j < SW_PF; ++j) bb[j] = 0xffffffffu;
            }
            // ---- fold tree t-1 in, second half: r -= new value of the leaf the observation ends up in
            const NodeS* const Ssel = L.S + (doPropose ? sset : 0) * SW_NC;
            if (doDecide && !bothHalves) {
              double muNew[SW_PF][4];
#pragma unroll
              for (int j = 0; j < SW_PF; ++j) {
#pragma unroll
                for (int e = 0; e < 4; ++e) muNew[j][e] = At[(toP[j] >> (8 * e)) & 63u].muNew;
              }
#pragma unroll
              for (int j = 0; j < SW_PF; ++j) {
#pragma unroll
                for (int e = 0; e < 4; ++e) O.r[j][e] -= muNew[j][e];
              }
            }
            // ---- statistics of tree t under the surviving proposal
            bool lastW = false;
            if (doPropose) {
              unsigned long long* const xCur = x.xbuf + (size_t)((nbSpec ? XC_RING : 0) + (t & (XC_RING - 1))) * XC_BUF_WORDS;   // (second ring: wave 3 had published this step's statistics already)
              double* const partOut = a.partF + (size_t)(t & 1) * 3 * a.binCap * a.gridF;
              for (int base = 0; base < nb; base += 8) {   // (8 bins per pass: sixteen accumulator pairs would not fit the registers beside the 16 observations)
                if (base > 0) pass_barrier(bar);     // the reduction slots are free again
                const int nbThis = nb - base < 8 ? nb - base : 8;
                lastW = sweep_stats_n<8, FEW, false, false, BATCH>(nbThis, a, L, bar, O.r, lfCur, Ssel, bb, q0p, stride, nQuads, base, xCur, partOut, bail, pw, lnP, 0, nullptr, nullptr, jMax);
              }
            }
            // (the wave that published — the last of the four to arrive at the reduction — says so)
            if (lastW && lnP == 0 && doPropose) { if (nbSpec) __hip_atomic_store(&F.publishedAlt, t + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); else __hip_atomic_store(&F.published, t + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }
#pragma unroll
            for (int j = 0; j < SW_PF; ++j) bbCur[j] = bb[j];     // (what the next step needs of this tree: its B bins under the proposal that was settled)
            if (!doPropose || bail) {   // the residual goes back to memory: end of the sweep, or the rest of it runs on k_step
#pragma unroll
              for (int j = 0; j < SW_PF; ++j) {
                const int64_t qd = q0p + (int64_t)j * stride;
                if (qd < nQuads) { const int64_t i0 = qd << 2; store_r(a.R + i0, O.r[j][0], O.r[j][1]); store_r(a.R + i0 + 2, O.r[j][2], O.r[j][3]); }
              }
            }
          }
          if (bail || !doPropose) break;
          // ---- the ahead pass for tree t+1 behind a step done the old way: the residual holds tree t-1 already (zero table), image 0 of tree t+1 is final
          if (!solo && haveNext) {
            if (!spin_counter(&F.img0Ready, t + 1, &F.abort)) { quit = true; break; }
            const CandSet c1 = cand_lds(L.img, t + 1, 0);
            const int idF = S4B_UNI(c1.meta[0]) != 0 ? S4B_UNI(c1.meta[3]) : 0;
            if (idF != 0) { if (idF != idNext) routeId = idF; run = true; nbNext = S4B_UNI(c1.head->pr.nbA) + S4B_UNI(c1.head->pr.nbB); }      // (run: if it has 1 .. 8 bins — below; the image is final: every wave reads the same header)
            else idNext = 0;
            foldD = reinterpret_cast<const double*>(L.zeroA);
          }
        }
        // ---- the B bins of tree t+1 under that image (one inlined copy of the routing for both phases)
        if (routeId != 0) {
          const CandSet c1 = cand_lds(L.img, t + 1, 0);
          const int set1 = 1 + sw_slot(t + 1, 0);
          if (hasObs) {
            const NodeS* const Ss[1] = {L.S + set1 * SW_NC};
            const NodeP* const SPs[1] = {L.SP + set1 * SW_NC};
            const int roots[1] = {S4B_UNI(c1.head->pr.node) & (SW_NC - 1)};
            const bool haves[1] = {true};
            unsigned bb1[1][SW_PF];
            sweep_route<1>(a, Ss, SPs, roots, haves, lfNext, q0p, stride, nQuads, bb1);
#pragma unroll
            for (int j = 0; j < SW_PF; ++j) bbNext[j] = bb1[0][j];
          }
          idNext = routeId;
        }
        if (phase == 0) { SW_D(2); }
        if (phase == 0) {
          // ---- did wave 3 publish the statistics of tree t (from the ahead pass of the step before)?  Then this step assumes "the move of tree t-1 is not
          // accepted, image 0 of tree t is its proposal" until the verdict says otherwise, and the ahead pass for tree t+1 runs now.
          if (spec) {
            if (!spin_counter(&F.linReady, t, &F.abort)) { quit = true; break; }
            nbSpec = __builtin_amdgcn_readfirstlane(F.specNb[t & 1]);
          }
          SW_D(3);
          run = nbSpec != 0 && idNext != 0 && nbNext >= 1 && nbNext <= 8;
        } else {
          run = run && nbNext >= 1 && nbNext <= 8;
          // (no barrier before the ahead pass: it uses neither the reduction slots nor anything another pass wave writes)
        }
        if (phase == 0 && t + 2 < T && hasObs) {      // (requested right in front of the ahead pass — 3 us of LDS and register work without a wait for the memory counter: every acquire of a flag, every release and the routing's own column loads wait for that counter, and wherever else this request stood its 2.5 us of memory latency showed up in the step — measured, round 6)
          const uint16_t* plane = a.leaf + (size_t)(t + 2) * a.npad;
#pragma unroll
          for (int j = 0; j < SW_PF; ++j) {
            const int64_t qd = q0p + (int64_t)j * stride;
            if (qd < nQuads) lfAfter[j] = __builtin_nontemporal_load(reinterpret_cast<const us4_t*>(plane + (qd << 2)));
          }
        }
        // ---- the ahead pass: pre-sums and contingency counts of tree t+1 (see LINEARITY)
        const int par1 = (t + 1) & 1;
        if (run && hasObs) {
          __builtin_amdgcn_s_setprio(S4B_PRIO_SPEC);
          if (pw == 1 && phase == 0) { SW_G(90); SW_W(9); }
          sweep_stats_n<8, FEW, true, false, BATCH>(nbNext, a, L, bar, O.r, lfNext, L.S + (1 + sw_slot(t + 1, 0)) * SW_NC, bbNext, q0p, stride, nQuads, 0, nullptr, nullptr, false, pw, lnP, 0,
                                      &O.lfPrev, nullptr, jMax, &lfCur, L.ctab + (size_t)par1 * SW_CT_WORDS, L.preS + par1 * SW_PW * 8, foldD);
          __builtin_amdgcn_s_setprio(0);
          ranAhead = true;
          if (phase == 0) { SW_D(4); }
        }
        if (phase == 1 || spec) {      // (no barrier inside the pass: the last of the four pass waves to arrive says it is done)
          // Everything the ahead pass leaves behind is in LDS, and a wave's LDS operations execute in the order it issued them: waiting for ITS OWN LDS counter orders its
          // pre-sums and counts before its arrival, and the last arriver's words before its flag.  (A release fence or store would also wait for the wave's outstanding
          // GLOBAL loads — the leaf ids requested a step ahead: 2 - 3 us of memory latency in front of wave 3's publish — measured, round 6.)
          // The arrival is a release fence all the same: with the wait for the wave's LDS counter alone in its place (s_waitcnt lgkmcnt(0), built and measured in
          // round 6) the chain differed from the oracle's in one run of four.
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          // (two branches, not a pointer chosen by the phase)
          if (lnP == 0 && phase == 0) {
            if (__hip_atomic_fetch_add(&F.preArrA, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == SW_PW - 1) {
              __hip_atomic_store(&F.preArrA, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              F.preNb[par1] = run ? nbNext : 0; F.preSeq[par1] = idNext;
              asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
              __hip_atomic_store(&F.preDoneA, t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
          } else if (lnP == 0) {
            if (__hip_atomic_fetch_add(&F.preArrB, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == SW_PW - 1) {
              __hip_atomic_store(&F.preArrB, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              F.preNb[par1] = run ? nbNext : 0; F.preSeq[par1] = idNext;
              asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
              __hip_atomic_store(&F.preDoneB, t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
          }
        }
      }
      if (quit) break;
      if (bailNow) { bailStep = t; break; }
      // ---- what the next step needs of these trees
#pragma unroll
      for (int j = 0; j < SW_PF; ++j) { O.lfPrev[j] = lfCur[j]; O.bbPrev[j] = bbCur[j]; lfCur[j] = lfNext[j]; bbCur[j] = bbNext[j]; lfNext[j] = lfq_pack(lfAfter[j]); }
      idCur = idNext;
      SW_MARK();
      if (ranAhead && nbSpec == 0) { SW_D(6); } else { SW_D0(); }      // (a step done the old way with its ahead pass behind it / the clock of the next step's first stamp)
      // (what this counter orders are this wave's LDS reads of the step: its own LDS counter, not a release — see the arrival above)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (lane == 0) __hip_atomic_fetch_add(&F.passSeen, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
#else
    SweepObs O;
    {
      SW_KERNARGS();
      const int64_t nQuads = (a.n + 3) >> 2;
#pragma unroll
      for (int j = 0; j < SW_PF; ++j) {
        const int64_t qd = q0 + (int64_t)j * stride;
        double2 r01 = make_double2(0.0, 0.0), r23 = make_double2(0.0, 0.0);
        if (hasObs && qd < nQuads) { const int64_t i0 = qd << 2; r01 = *reinterpret_cast<const double2*>(a.R + i0); r23 = *reinterpret_cast<const double2*>(a.R + i0 + 2); }
        O.r[j][0] = r01.x; O.r[j][1] = r01.y; O.r[j][2] = r23.x; O.r[j][3] = r23.y;
        O.lfPrev[j] = 0u; O.bbPrev[j] = 0xffffffffu;
      }
    }
    const int64_t q0w = q0;
    for (int t = 0; t <= T; ++t) {
      const bool doDecide = t > 0, doPropose = t < T;
      const int tn = doPropose ? t : 0;
      const bool spec = doDecide && doPropose;
      SW_KERNARGS();
      const int64_t nQuads = (a.n + 3) >> 2;
      // (the thread's first quad, opaque once per step: the sixteen 64-bit observation indices derived from it are otherwise kept across the
      // steps — 32 registers the residual and the statistics need, i.e. spills)
      int64_t q0 = q0w;
      asm volatile("" : "+v"(q0));
      // quads the threads of this workgroup own at most (thread 0 owns the most): a launch over few observations skips the unrolled work of the others
      int jMax = 0;
#pragma unroll
      for (int j = 0; j < SW_PF; ++j) jMax += ((int64_t)SW_BX * SW_PT + (int64_t)j * stride < nQuads) ? 1 : 0;
      jMax = __builtin_amdgcn_readfirstlane(jMax);
      // ---- the statistics half, as far as it does not depend on the pending decision: leaf ids of the observations in tree tn,
      // their A bins and leaf values, and their B bins under image 0 of the tree's proposal
      lfq_t lf[SW_PF]; unsigned bbI[1][SW_PF];
      bool have0 = false;
#pragma unroll
      for (int j = 0; j < SW_PF; ++j) { lf[j] = 0u; bbI[0][j] = 0xffffffffu; }
      if (doPropose && hasObs) {
        const uint16_t* plane = a.leaf + (size_t)tn * a.npad;
#pragma unroll
        for (int j = 0; j < SW_PF; ++j) {
          const int64_t qd = q0 + (int64_t)j * stride;
          if (qd < nQuads) lf[j] = lfq_pack(__builtin_nontemporal_load(reinterpret_cast<const us4_t*>(plane + (qd << 2))));
        }
      }
      // ---- wave 4: tree t+1, main arrays -> stage (the image waves propose for it during this step)
      if (pw == 0 && doPropose) {      // trees are staged two steps before they are decided (the image waves draw one step ahead)
        if (t == 0 && T > 1) stage_tree(a, L.stage, 1, lane);
        // (its stage is the one of tree t-1: wave 2 may still be drawing image 1 of that tree from it — since round 6 the verdict no longer waits for an image 1 it does not need)
        if (t + 2 < T) { if (t >= 1) spin_counter(&F.img1Ready, t - 1, &F.abort); stage_tree(a, L.stage, t + 2, lane); }
        if (lane == 0) __hip_atomic_store(&F.staged, t + 2 < T ? t + 2 : T - 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      if (doPropose && hasObs && spec) {
#ifdef S4B_SWEEP_TIMING
        const long long tImgWait = wall_clock64();
#endif
        // (image 0 only — final since the step before last in a chain that rejects, i.e. nearly always: an accepted birth / death routes
        // under its own image after the verdict, like a proposal wave 0 had to draw itself)
        if (spin_counter(&F.img0Ready, tn, &F.abort)) {
          if (pw == 0) SW_T(2);
#ifdef S4B_SWEEP_TIMING
          const long long tImgSeen = wall_clock64();
#endif
          const CandSet c0 = cand_lds(L.img, tn, 0);
          have0 = S4B_UNI(c0.meta[0]) != 0;
          const int set0 = 1 + sw_slot(tn, 0);
          if (have0) {
            const NodeS* const Ss[1] = {L.S + set0 * SW_NC};
            const NodeP* const SPs[1] = {L.SP + set0 * SW_NC};
            const int roots[1] = {S4B_UNI(c0.head->pr.node)};
            const bool haves[1] = {true};
            unsigned bb1[1][SW_PF];
            sweep_route<1>(a, Ss, SPs, roots, haves, lf, q0, stride, nQuads, bb1);
#pragma unroll
            for (int j = 0; j < SW_PF; ++j) bbI[0][j] = bb1[0][j];
          }
          if (pw == 0) SW_T(3);
          if (pw == 1) {  SW_AP(44); }
#ifdef S4B_SWEEP_TIMING
          if ((int)SW_BX == SW_TIMED_WG && lane == 0 && t > 0 && t < T && pw == 1 && __hip_atomic_load(&F.foldReady, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= t) {
            atomicAdd(&F.tacc[55], 1ull); atomicAdd(&F.tacc[56], (unsigned long long)(wall_clock64() - F.tFold));
            atomicAdd(&F.tacc[57], (unsigned long long)(wall_clock64() - tImgSeen)); atomicAdd(&F.tacc[58], (unsigned long long)(tImgSeen - F.t0[t & 3]));
            atomicAdd(&F.tacc[59], (unsigned long long)(F.bothStep == t ? 1 : 0));
            atomicAdd(&F.tacc[28], (unsigned long long)(tImgSeen - tImgWait));
            atomicAdd(&F.tacc[20 + (cand_lds(L.img, tn, 0).head->pr.type & 3)], 1ull); }
          else if ((int)SW_BX == SW_TIMED_WG && lane == 0 && t > 0 && t < T && pw == 1) {
            atomicAdd(&F.tacc[60], (unsigned long long)(wall_clock64() - tImgSeen)); atomicAdd(&F.tacc[61], (unsigned long long)(tImgSeen - F.t0[(t - 1) & 3])); }
#endif
        }
      }
      // ---- SPECULATION: "the move of tree t-1 is not accepted and image 0 of tree t is its proposal" (77 % of the steps of a cold chain, 98 % of
      // a stationary one).  Everything that outcome needs is known 1.3 us after the totals — wave 3's leaf values, the routing under image 0 —,
      // the accept test takes 2.4 us and the settled proposal 3.0: the statistics of tree t are gathered from the residual with tree t-1 folded
      // in ON THE FLY (the residual itself stays as it is) and PUBLISHED, into the first ring, without waiting for the decider; the exchange
      // runs beside the accept test.  When the verdict bears the outcome out, the residual is folded the same way (same operations in the
      // same order as below: the same bits) and the step is over; otherwise the statistics are gathered again and go to the second ring,
      // where every workgroup — they all see the same verdict — then looks for the totals.
      const NodeA* const At = L.A + (t & 1) * SW_NC;      // leaf-value table of this step
      int nbSpec = 0;
      if (doDecide && doPropose) {
        int guard = 0, sp;
        while (((sp = __hip_atomic_load(&F.specReady, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) >> 1) < t) {
          __builtin_amdgcn_s_sleep(SW_SLEEP);
          if (++guard > (1 << 21) || (((guard & 1023) == 0) && __hip_atomic_load(&F.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))) {
            int none = 0; __hip_atomic_compare_exchange_strong(&F.abort, &none, __LINE__, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); break; }
        }
        if (__hip_atomic_load(&F.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
        nbSpec = __builtin_amdgcn_readfirstlane(F.specNb[t & 1]);      // (one reader of the image for all: the verdict may overwrite it any time from here)
        if (nbSpec && hasObs) {
          __builtin_amdgcn_s_setprio(S4B_PRIO_SPEC);
          if (pw == 1) { SW_G(90); SW_W(9); }
          const bool lastS = sweep_stats_n<8, FEW, false, WT, BATCH>(nbSpec, a, L, bar, O.r, lf, L.S + (1 + sw_slot(tn, 0)) * SW_NC, bbI[0], q0, stride, nQuads, 0,
                           x.xbuf + (size_t)(t & (XC_RING - 1)) * XC_BUF_WORDS, nullptr, false, pw, lane, 0, &O.lfPrev, At, jMax,
                           nullptr, nullptr, nullptr, nullptr, wLds + (size_t)pt * 4, nbSpec, x.wScale);
          if (lastS) { if (lane == 0 && !solo) __hip_atomic_store(&F.published, t + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); SW_A(50); SW_G(91);
#ifdef S4B_SWEEP_WG
            if (lane == 0 && t > 0 && t < T && (int)SW_BX < 256) {
              const unsigned long long nw = (unsigned long long)wall_clock64();
              atomicAdd(&g_wg[SW_BX * 16], nw - (unsigned long long)F.t0[t & 3]); atomicAdd(&g_wg[SW_BX * 16 + 1], 1ull);
              atomicMax(&g_pubMax[t & 7], nw); atomicMin(&g_pubMin[t & 7], nw);
            }
#endif
          }
          __builtin_amdgcn_s_setprio(0);
#ifdef S4B_SWEEP_TIMING
          if ((int)SW_BX == SW_TIMED_WG && lane == 0 && pw == 0 && t < T) atomicAdd(&g_sw[89], 1ull);
#endif
        }
      }
      // ---- the verdict is out: old leaf values, which observations move and where to — fold the old values in, relabel
      bool bothHalves = false;
      unsigned toP[SW_PF];      // node the observation ends up in (one byte per observation)
#pragma unroll
      for (int j = 0; j < SW_PF; ++j) toP[j] = 0u;
      if (doDecide) {
        spin_counter(&F.foldReady, t, &F.abort);
#ifdef S4B_SWEEP_TIMING
        if ((int)SW_BX == SW_TIMED_WG && lane == 0 && t > 0 && t < T && pw <= 1) atomicAdd(&F.tacc[53 + pw], (unsigned long long)(wall_clock64() - F.tFold));
#endif
        if (pw == 1) SW_A(45);
        bothHalves = __builtin_amdgcn_readfirstlane(F.bothStep) == t;
        if (nbSpec) {
          if (pw == 1) SW_G(92);
          spin_counter(&F.tablesReady, t, &F.abort);
          spin_counter(&F.paGo, t + 1, &F.abort);
          if (__hip_atomic_load(&F.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
          if (sweep_spec_confirmed(F, t, nbSpec)) {
            // (unreachable: the exchange wave sets specNbPre, hence nbSpec, only `if (... && !solo)`.  Kept because removing it moves register allocation and scheduling all over
            // k_sweep*, which needs a measured A/B of its own — DESIGN.md 5.0)
            if (solo && pw == 0) {
              const int ln = sweep_fresh_lane();
              if ((ln & 7) == 0 && (ln >> 3) < nbSpec) { bar.totS[ln >> 3] = 0.0; bar.totC[ln >> 3] = 0.0; }
              if (ln == 0) __hip_atomic_store(&F.published, t + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            if (hasObs) {
#pragma unroll
              for (int j = 0; j < SW_PF; ++j) {
                const unsigned pl[4] = LFQ4(O.lfPrev[j]);
                NodeA na[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) na[e] = At[pl[e] & 63u];
#pragma unroll
                for (int e = 0; e < 4; ++e) { O.r[j][e] += na[e].muOld; O.r[j][e] -= na[e].muNew; }
              }
#pragma unroll
              for (int j = 0; j < SW_PF; ++j) { O.lfPrev[j] = lf[j]; O.bbPrev[j] = bbI[0][j]; }
              if (pw == 0) { SW_T(6);
#ifdef S4B_SWEEP_TIMING
                if ((int)SW_BX == SW_TIMED_WG && lane == 0 && t > 0 && t < T) { atomicAdd(&F.tacc[0], 1ull); atomicAdd(&F.tacc[7], (unsigned long long)nbSpec); atomicAdd(&g_sw[72 + (nbSpec < 15 ? nbSpec : 15)], 1ull); atomicAdd(&g_sw[88], 1ull); }
#endif
              }
            }
            if (pw == 1) { SW_G(93); SW_W(11); }
            SW_MARK();
            if (lane == 0) __hip_atomic_fetch_add(&F.passSeen, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            continue;
          }
          if (hasObs) pass_barrier(bar);     // (not borne out: the reduction slots are free again once every pass wave is here)
        }
        if (hasObs && bothHalves) {
          // the move was not accepted and both halves of the leaf-value table came with the verdict: nobody moves, one 16-byte read
          // per observation, the same two operations in the same order as below
#pragma unroll
          for (int j = 0; j < SW_PF; ++j) {
            const unsigned pl[4] = LFQ4(O.lfPrev[j]);
            NodeA na[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) na[e] = At[pl[e] & 63u];
#pragma unroll
            for (int e = 0; e < 4; ++e) { O.r[j][e] += na[e].muOld; O.r[j][e] -= na[e].muNew; }
          }
        } else if (hasObs) {
          const int prevAcc = __builtin_amdgcn_readfirstlane(F.prevAcc), prevRoot = __builtin_amdgcn_readfirstlane(F.prevRoot), prevDeath = __builtin_amdgcn_readfirstlane(F.prevDeath);
          const unsigned accM = sw_mask(prevAcc != 0), deathM = sw_mask(prevDeath != 0);
          uint16_t* const prevPlane = a.leaf + (size_t)(t - 1) * a.npad;
#pragma unroll
          for (int j = 0; j < SW_PF; ++j) {
            const int64_t qd = q0 + (int64_t)j * stride;
            const int valid = qd < nQuads ? ((a.n - (qd << 2)) >= 4 ? 4 : (int)(a.n - (qd << 2))) : 0;
            const unsigned pl[4] = LFQ4(O.lfPrev[j]);
            // every table read unconditional, every index valid either way (leaf ids beyond n are 0: those residuals are never
            // used), results merged with opaque masks: all reads of the thread's 16 observations are in flight together
            double muOld[4]; unsigned ain[4], via[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              muOld[e] = At[pl[e]].muOld; ain[e] = L.Ain[pl[e]];
              via[e] = L.b2n[(O.bbPrev[j] >> (8 * e)) & 63u];
            }
            unsigned nl[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const unsigned m = (0u - (unsigned)(ain[e] != 0u)) & accM;
              nl[e] = sw_sel(m, sw_sel(deathM, (unsigned)prevRoot, via[e]), pl[e]) & 63u;
              O.r[j][e] += muOld[e];
            }
            toP[j] = nl[0] | (nl[1] << 8) | (nl[2] << 16) | (nl[3] << 24);
            if (prevAcc && valid > 0) { us4_t o4; o4.x = (unsigned short)nl[0]; o4.y = (unsigned short)nl[1]; o4.z = (unsigned short)nl[2]; o4.w = (unsigned short)nl[3];
                                        __builtin_nontemporal_store(o4, reinterpret_cast<us4_t*>(prevPlane + (qd << 2))); }
          }
        }
      }
      if (pw == 1) SW_A(46);
      // ---- the leaf values of tree t-1 are out and the proposal of tree tn is settled
      if (doDecide) spin_counter(&F.tablesReady, t, &F.abort);
      if (doPropose) spin_counter(&F.paGo, t + 1, &F.abort);
      if (__hip_atomic_load(&F.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
      if (pw == 0) SW_T(4);
      if (pw == 1) {  SW_A(47); }
      const int root = __builtin_amdgcn_readfirstlane(F.root), nb = doPropose ? __builtin_amdgcn_readfirstlane(F.nb) : 0, sset = __builtin_amdgcn_readfirstlane(F.sset);
      const bool bail = doPropose && __builtin_amdgcn_readfirstlane(F.needBig) != 0;
      if (hasObs) {
        // the B bins under the surviving proposal; when it is none of the two images (wave 0 proposed itself), route now
        unsigned bb[SW_PF];
        const int set0 = 1 + sw_slot(tn, 0);
        if (doPropose && sset == set0 && have0) {
#pragma unroll
          for (int j = 0; j < SW_PF; ++j) bb[j] = bbI[0][j];
        } else if (doPropose) {
#ifdef S4B_SWEEP_TIMING
          if ((int)SW_BX == SW_TIMED_WG && pw == 0 && lane == 0 && t > 0) atomicAdd(&F.tacc[8], 1ull);
#endif
          const NodeS* Sx = L.S + sset * SW_NC;
          {
            const NodeS* const Ss[1] = {Sx}; const NodeP* const SPs[1] = {L.SP + sset * SW_NC}; const int roots[1] = {root}; const bool haves[1] = {true};
            unsigned bb1x[1][SW_PF];
            sweep_route<1>(a, Ss, SPs, roots, haves, lf, q0, stride, nQuads, bb1x);
#pragma unroll
            for (int j = 0; j < SW_PF; ++j) bb[j] = bb1x[0][j];
          }
        } else {
#pragma unroll
          for (int j = 0; j < SW_PF; ++j) bb[j] = 0xffffffffu;
        }
        // ---- fold tree t-1 in, second half: r -= new value of the leaf the observation ends up in
        const NodeS* const Ssel = L.S + (doPropose ? sset : 0) * SW_NC;
        if (doDecide && !bothHalves) {
          double muNew[SW_PF][4];
#pragma unroll
          for (int j = 0; j < SW_PF; ++j) {
#pragma unroll
            for (int e = 0; e < 4; ++e) muNew[j][e] = At[(toP[j] >> (8 * e)) & 63u].muNew;
          }
#pragma unroll
          for (int j = 0; j < SW_PF; ++j) {
#pragma unroll
            for (int e = 0; e < 4; ++e) O.r[j][e] -= muNew[j][e];
          }
        }
        if (pw == 0) SW_T(5);
        if (pw == 1) {  SW_A(48); }
        SW_T(16 + pw);
        // ---- statistics of tree tn under the surviving proposal
        bool lastW = false;
        if (doPropose) {
          unsigned long long* const xCur = x.xbuf + (size_t)((nbSpec ? XC_RING : 0) + (t & (XC_RING - 1))) * XC_BUF_WORDS;   // (second ring: after a speculation that failed)
          double* const partOut = a.partF + (size_t)(t & 1) * 3 * a.binCap * a.gridF;
          for (int base = 0; base < nb; base += 8) {   // (8 bins per pass: sixteen accumulator pairs would not fit the registers beside the 16 observations)
            if (base > 0) pass_barrier(bar);     // the reduction slots are free again
            const int nbThis = nb - base < 8 ? nb - base : 8;
            lastW = sweep_stats_n<8, FEW, false, WT, BATCH>(nbThis, a, L, bar, O.r, lf, Ssel, bb, q0, stride, nQuads, base, xCur, partOut, bail, pw, lane,
#ifdef S4B_SWEEP_TIMING
                             (t > 0 && t < T) ? tStep : 0,
#else
                             0,
#endif
                             nullptr, nullptr, jMax, nullptr, nullptr, nullptr, nullptr, wLds + (size_t)pt * 4, nb, x.wScale);
          }
        }
        if (lastW && lane == 0 && doPropose) __hip_atomic_store(nbSpec ? &F.publishedAlt : &F.published, t + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (pw == 0) SW_A(50);
        if (pw == 1) {  SW_A(49); }
        // what the next step needs of this tree
#pragma unroll
        for (int j = 0; j < SW_PF; ++j) { O.lfPrev[j] = lf[j]; O.bbPrev[j] = bb[j]; }
        if (pw == 0) { SW_T(6);
#ifdef S4B_SWEEP_TIMING
          if ((int)SW_BX == SW_TIMED_WG && lane == 0 && t > 0 && t < T) { atomicAdd(&F.tacc[0], 1ull); atomicAdd(&F.tacc[7], (unsigned long long)nb); atomicAdd(&g_sw[72 + (nb < 15 ? nb : 15)], 1ull); }    // [72..87] histogram of the bins per step
#endif
        }
        SW_MARK();
        if (!doPropose || bail) {   // the residual goes back to memory: end of the sweep, or the rest of it runs on k_step
#pragma unroll
          for (int j = 0; j < SW_PF; ++j) {
            const int64_t qd = q0 + (int64_t)j * stride;
            if (qd < nQuads) { const int64_t i0 = qd << 2; store_r(a.R + i0, O.r[j][0], O.r[j][1]); store_r(a.R + i0 + 2, O.r[j][2], O.r[j][3]); }
          }
        }
      }
      if (bail) { bailStep = t; break; }
      if (lane == 0) __hip_atomic_fetch_add(&F.passSeen, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
#endif   // S4B_LINEAR
    }   // (!STREAM)
  }
  // ======================================================================================== end of the launch
  if (__hip_atomic_load(&F.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {   // a wait timed out: the status word stays at -1
    SW_KERNARGS();
    if (threadIdx.x == 0) { *a.errFlag |= S4B_ERR_INTERNAL | S4B_ERR_I_WAIT; x.status[1] = F.abort; }
    return;
  }
  __syncthreads();
#ifdef S4B_SWEEP_TIMING
  if ((int)SW_BX == SW_TIMED_WG && threadIdx.x < 64 && F.tacc[threadIdx.x]) atomicAdd(&g_sw[threadIdx.x], F.tacc[threadIdx.x]);
#endif
  if (F.abort) { SW_KERNARGS(); if (threadIdx.x == 0) { *a.errFlag |= S4B_ERR_INTERNAL | S4B_ERR_I_WAIT; x.status[1] = F.abort; } return; }
#ifdef S4B_TUNING
  { SW_KERNARGS(); if (threadIdx.x == 0 && SW_BX < 6) x.status[2 + SW_BX] = (F.needBig << 24) | (F.paGo << 8) | (bailStep & 0xff); }
#endif
  if (!F.needBig) {
    SW_KERNARGS();
    if (ctl && threadIdx.x == 0) *x.status = T + 1;
    return;
  }
  {
    // ==================================================================== hand-over to k_step: launch t+1 finds what launch t would have left
    SW_KERNARGS();
    const int t = __builtin_amdgcn_readfirstlane(F.paGo) - 1;     // the step that found the next control step too large (every wave left its loop there)
    (void)bailStep;
    const int tn = t;
    const int nc = a.nc;
    const int G = (int)SW_GX;
    double* const partOut = a.partF + (size_t)(t & 1) * 3 * a.binCap * a.gridF;
    const size_t kindStride = (size_t)a.binCap * a.gridF;
    if (ctl) {
      const int sel = F.selSlot[tn & 1];
      const CandSet cw = cand_lds(L.img, tn, sel);
      const StepScratch& cN = a.sc[tn & 1];
      if (wv == 3) {
        if (lane < SW_NC && lane < nc) {
#pragma unroll
          for (int r = 0; r < SF_COUNT; ++r) cN.slab[r * nc + lane] = cw.slab[r * SW_NC + lane];
          cN.insub[lane] = cw.insub[lane]; cN.snapMu[lane] = cw.snapMu[lane]; cN.snapCnt[lane] = cw.snapCnt[lane];
        }
        if (lane < 28) ((int32_t*)cN.head)[lane] = ((const int32_t*)cw.head)[lane];
      }
      if (wv == 4) {
        MTState* rngOut = a.rngF + ((t + 1) & 1);
#pragma unroll
        for (int j = 0; j < MTJ; ++j) { const int i = lane + j * 64; if (i < MTW) ((uint32_t*)rngOut)[i] = ((const uint32_t*)cw.rng)[i]; }
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const int k = __hip_atomic_fetch_add(a.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      F.last = (k == G - 1) ? 1 : 0;
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#ifdef S4B_TUNING
      x.status[8 + (SW_BX & 3)] = 1000 + k;
#endif
    }
    __syncthreads();
    if (!F.last) return;
    {
#ifdef S4B_TUNING
      if (threadIdx.x == 0) x.status[12] = 1;
#endif
      const int nbAll = F.nb, grid = a.gridF;
      for (int k = wv; k < nbAll; k += FBLOCK / 64) {
        double sm = 0.0, c = 0.0, wt = 0.0;
        // (solo: workgroup 0 wrote the partial of ALL observations; the slots of the other pass workgroups of k_step's geometry are stale)
        for (int b = lane; b < (solo ? 1 : grid - 1); b += 64) { sm += partOut[(size_t)k * grid + b]; c += partOut[kindStride + (size_t)k * grid + b]; if (WT) wt += partOut[2 * kindStride + (size_t)k * grid + b]; }
        sm = wave_sum(sm); c = wave_sum(c); if (WT) wt = wave_sum(wt);
        if (lane == 0) { a.binSum[k] = sm; a.binCnt[k] = c; if (WT) a.binWt[k] = wt; }
      }
      MTState* rngNext = a.rngF + (t & 1);
      const MTState* rngCur = a.rngF + ((t + 1) & 1);
      for (int i = threadIdx.x; i < MTW; i += FBLOCK) ((uint32_t*)rngNext)[i] = ((const uint32_t*)rngCur)[i];
      cache_to_main(a, tn);
      __threadfence();
      __syncthreads();
      const int next = t + 1 < T ? t + 1 : -1;
#ifdef S4B_TUNING
      if (threadIdx.x == 0) x.status[12] = 2;
#endif
      if (threadIdx.x == 0) { BartArrays b = a; b.rng = rngNext; b.rng->pad = 0; control_global_path(b, tn, next, S.scratch[0]); }
#ifdef S4B_TUNING
      if (threadIdx.x == 0) x.status[12] = 3;
#endif
      __threadfence();
      __syncthreads();
      if (next >= 0) snapshot_from_main(a, next);
      if (threadIdx.x == 0) { a.preDone[(t + 1) & 1] = 1; *a.ticket = 0; __threadfence(); *x.status = t + 1; }
    }
  }
}
__global__ __launch_bounds__(FBLOCK) void k_sweep(BartArrays aKern, SweepArgs xKern) { sweep_body<false, false>(aKern, xKern); }
// (the same launch for few observations: no pass thread owns all SW_PF quads, the statistics leave the unrolled work of the missing ones out)
__global__ __launch_bounds__(FBLOCK) void k_sweep_few(BartArrays aKern, SweepArgs xKern) { sweep_body<false, true>(aKern, xKern); }
__global__ __launch_bounds__(FBLOCK) void k_sweep_stream(BartArrays aKern, SweepArgs xKern) { sweep_body<true, false>(aKern, xKern); }
// (cgm(split.probs): the same launches with the weighted predictor choice compiled into the wave-register control code — WaveModelT<true>, dev_control.hpp)
__global__ __launch_bounds__(FBLOCK) void k_sweep_sp(BartArrays aKern, SweepArgs xKern) { sweep_body<false, false, true>(aKern, xKern); }
__global__ __launch_bounds__(FBLOCK) void k_sweep_few_sp(BartArrays aKern, SweepArgs xKern) { sweep_body<false, true, true>(aKern, xKern); }
#if !S4B_LINEAR
// (observation weights: sweep_stats<.., WT>.  One kernel for every size: the instantiation without the skipped quads — three accumulators per bin unrolled over
// four quads — spills 878 registers; the one with them, which the compiler does not interleave across the quads, none)
__global__ __launch_bounds__(FBLOCK) void k_sweep_w(BartArrays aKern, SweepArgs xKern) { sweep_body<false, true, false, true>(aKern, xKern); }
#else
__global__ __launch_bounds__(FBLOCK) void k_sweep_w(BartArrays, SweepArgs xKern) { if (threadIdx.x == 0 && blockIdx.x == 0) *xKern.status = -3; }      // (the linear variant has no weighted sweep: refused, the host raises an error)
#endif
// Batched launches of the solo sweep (the sweep group, dev_hip.hip): workgroup b is member b's one-workgroup sweep, its arguments in slot b.
// No workgroup of such a launch waits for another one.
__global__ __launch_bounds__(FBLOCK) void k_sbatch(const unsigned char*) { sweep_body<false, false, false, false, true>(0, 0); }
__global__ __launch_bounds__(FBLOCK) void k_sbatch_few(const unsigned char*) { sweep_body<false, true, false, false, true>(0, 0); }
__global__ __launch_bounds__(FBLOCK) void k_sbatch_sp(const unsigned char*) { sweep_body<false, false, true, false, true>(0, 0); }
__global__ __launch_bounds__(FBLOCK) void k_sbatch_few_sp(const unsigned char*) { sweep_body<false, true, true, false, true>(0, 0); }
#if !S4B_LINEAR
__global__ __launch_bounds__(FBLOCK) void k_sbatch_w(const unsigned char*) { sweep_body<false, true, false, true, true>(0, 0); }
#else
__global__ __launch_bounds__(FBLOCK) void k_sbatch_w(const unsigned char* slots) {      // (as k_sweep_w in the linear variant: refused; the host never batches a weighted member there)
  if (threadIdx.x == 0) *((const SweepArgs*)(slots + (size_t)blockIdx.x * SW_SLOT_BYTES + SW_SLOT_XOFF))->status = -3;
}
#endif
}  // namespace s4b
