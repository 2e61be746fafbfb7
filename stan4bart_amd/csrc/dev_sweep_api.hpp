// What the host driver (dev_hip.hip) needs of the persistent sweep, whose kernels are compiled in dev_sweep.hip: the argument struct,
// the geometry constants and LDS sizes of a launch, the slot layout of a batched launch, the kernels' declarations and the read-out
// functions of the measurement builds.  dev_sweep.hip includes it too, so every one of these is declared once.
#ifndef S4B_DEV_SWEEP_API_HPP
#define S4B_DEV_SWEEP_API_HPP

#include "dev_step_shared.hpp"

#if defined(S4B_SWEEP_TIMING) || defined(S4B_SWEEP_WGT) || defined(S4B_SWEEP_WGD)
#define S4B_SWEEP_WG 1     // per-workgroup stamps of the exchange (dev_sweep.inc: SW_W)
#endif

// LINEAR statistics (round 6; see "LINEARITY" at the pass waves): the O(N) statistics pass of tree t+1 runs one step AHEAD, over the residual with
// tree t still missing, and gathers beside the bin sums the integer CONTINGENCY counts (leaf of tree t) x (bin of tree t+1); when the leaf values
// of tree t arrive, the exchange wave turns both into the workgroup's statistics with (leaves x bins) multiply-adds and publishes them itself.
// Built, parity-green against the oracle over the whole GPU suite, measured — and NOT the default (gate of VERDICT r05 item 1: "if the step does not drop by
// >= 1.2 us, record and stop"): 9.0 us per tree update in the benchmark's stationary chain against 8.45 for the statistics on the chain (profiles/r06_linear_gate.txt;
// the pass waves' work per step — route 2.0 + ahead pass 3.0 + fold — and one proposal drawing per step on wave 1 become the bound once the
// exchange no longer is).  `make linear` builds libs4b_linear.so; tests/test_gpu_linear.py keeps it under the oracle.
#ifndef S4B_LINEAR
#define S4B_LINEAR 0
#endif

namespace s4b {

constexpr int SW_NC = 64;            // node slots of the wave-register control path = row length of the on-chip tables
constexpr int SW_PW = 4;             // pass waves (4..7): one per SIMD
constexpr int SW_PT = SW_PW * 64;    // pass threads per workgroup
constexpr int SW_PF = 4;             // quads per pass thread (16 observations), all of them in registers for the whole sweep
constexpr unsigned long long SW_ROLL_GO = 1ull, SW_ROLL_BUSY = 2ull;
constexpr int XC_ROLL_WORDS = 8;     // words behind each exchange ring: [0] tickets of the roll call, [1] its decision
constexpr int SW_SETS = 6;           // statistics-half table sets: 0 wave 0's own proposal, 1 + sw_slot(tree, c) image c of the tree
constexpr int SW_SLOTS = 5;          // image slots: image 0 of tree t in slot t % 3 (it is drawn one step AHEAD), image 1 in slot 3 + (t & 1)
constexpr int SW_STAGES = 3;         // staged trees: tree t in stage t % 3 (staged two steps before it is decided)
constexpr int SW_CC = 4;                               // copies of every contingency count: lane & 3 picks one (lanes of a wave with the same key spread over four banks)
constexpr int SW_CT_WORDS = SW_NC * 8 * SW_CC + 16;    // counts [node of tree t][bin of tree t+1][copy] + a row of dummies for the observations that are in no bin
struct SweepArgs { unsigned long long* xbuf; int32_t* status; unsigned long long* xnext; double wScale, wUnscale; };   // (wScale / wUnscale: observation weights, k_sweep_w — a power of two and its inverse)   // exchange ring [XC_RING][XC_COPIES][XC_WORDS]; host-visible status word; the ring of the NEXT launch (cleared by this one)

// tree t as the main arrays hold it, staged in LDS one step before a wave proposes for it
struct __attribute__((aligned(16))) TreeStage { int16_t row[TF_COUNT][SW_NC]; double mu[SW_NC]; int32_t cnt[SW_NC]; int32_t sc[TI_COUNT]; int32_t pad0[2]; double logPi; };
constexpr int SW_RED_ROW = SW_PT + 8;   // per-thread partials of one bin, one row per bin (padded: the rows of the 8 bins start 16 banks apart)
__host__ __device__ static inline size_t stage_bytes() { return (sizeof(TreeStage) + 15) / 16 * 16; }
__host__ __device__ static inline size_t sweep_lds_bytes() {
  return (size_t)SW_SETS * SW_NC * 24 + (size_t)2 * SW_NC * 16 + 64 + 64 + (size_t)8 * SW_RED_ROW * 12 + SW_SLOTS * cand_bytes(SW_NC) + SW_STAGES * stage_bytes() + (size_t)SW_NC * 24 +
         (size_t)2 * SW_CT_WORDS * 4 + (size_t)2 * SW_PW * 8 * 8 + (size_t)2 * 8 * 4 + (size_t)SW_NC * 16 + (size_t)2 * SW_NC * 8;
}
// one member's slot of a batched launch (sweep_batch.inc): its BartArrays, then its SweepArgs at the offset SW_KERNARGS reads them from
constexpr size_t SW_SLOT_XOFF = (sizeof(BartArrays) + 7) / 8 * 8;
constexpr size_t SW_SLOT_BYTES = (SW_SLOT_XOFF + sizeof(SweepArgs) + 255) / 256 * 256;
static_assert(SW_SLOT_XOFF == (sizeof(BartArrays) + 7) / 8 * 8, "slot layout = kernarg layout");

__global__ __launch_bounds__(FBLOCK) void k_sweep(BartArrays aKern, SweepArgs xKern);
__global__ __launch_bounds__(FBLOCK) void k_sweep_stream(BartArrays aKern, SweepArgs xKern);
__global__ __launch_bounds__(FBLOCK) void k_sweep_few(BartArrays aKern, SweepArgs xKern);
__global__ __launch_bounds__(FBLOCK) void k_sweep_sp(BartArrays aKern, SweepArgs xKern);
__global__ __launch_bounds__(FBLOCK) void k_sweep_few_sp(BartArrays aKern, SweepArgs xKern);
__global__ __launch_bounds__(FBLOCK) void k_sweep_w(BartArrays aKern, SweepArgs xKern);
__global__ __launch_bounds__(FBLOCK) void k_sbatch(const unsigned char* slots);
__global__ __launch_bounds__(FBLOCK) void k_sbatch_few(const unsigned char* slots);
__global__ __launch_bounds__(FBLOCK) void k_sbatch_sp(const unsigned char* slots);
__global__ __launch_bounds__(FBLOCK) void k_sbatch_few_sp(const unsigned char* slots);
__global__ __launch_bounds__(FBLOCK) void k_sbatch_w(const unsigned char* slots);      // (a stub in the linear variant, which has no k_sweep_w: never launched there)
// (measurement builds: each reads and clears)
void sweep_timing_fetch(unsigned long long* out);
void sweep_decide_fetch(unsigned long long* out);
void sweep_wg_fetch(unsigned long long* out);
void sweep_wd_fetch(unsigned long long* out);

}  // namespace s4b
#endif
