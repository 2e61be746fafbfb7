// Host orchestration of one chain of the blocked Gibbs sampler on top of a device layer.
//
// Mirrors the reference's C++ driver — `Sampler` (reference src/init.cpp:124-173), createSampler
// (:190-310) and run (:678-965, loop body :752-917) — with the two blocks re-targeted:
//   * BART block: device-resident (DevLayer::sweep); nothing O(N) crosses PCIe inside the loop.
//   * Stan block: NUTS control flow on the host (stan_host.hpp), O(N) sums on the device, by default
//     folded into sufficient statistics once per Gibbs iteration.
// `Dev` is the device layer.  The product instantiates it with the HIP layer (dev_hip.hip); a CPU
// emulation of the same interface exists only under tests/emul to exercise this file without a GPU.
#ifndef S4B_SAMPLER_CORE_HPP
#define S4B_SAMPLER_CORE_HPP

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/stan4bart_amd.h"
#include "sweep_group.hpp"
#include "dev_common.hpp"
#include "stan_host.hpp"

namespace s4b {

enum { OFFSET_DEFAULT = 0, OFFSET_FIXEF, OFFSET_RANEF, OFFSET_BART, OFFSET_PARAMETRIC };
enum { OBS_R = 0, OBS_OFF, OBS_LAT, OBS_Y };   // observation-length device arrays addressable through download_obs / upload_obs

// a node of a kept tree (predict): children are slot ids relative to the tree's first record
struct PackedNode { int16_t var; uint16_t cut; int16_t left, right; double mu; int32_t n; int32_t pad; };   // n: observations in the node

// everything the device layer needs at creation (host pointers, valid during init() only)
struct DevInit {
  int64_t n = 0, nTest = 0; int32_t P = 0, T = 0, nc = 256, device = 0;
  const uint16_t* xbin = nullptr;      // [P][n]
  const uint16_t* xbinTest = nullptr;  // [P][nTest]
  const int32_t* numCuts = nullptr;
  const double* y = nullptr;
  const double* userOffset = nullptr;
  const double* weights = nullptr;     // [n] or null
  ModelView model;
  int32_t K = 0, q = 0, binary = 0;
  const double* X = nullptr;           // n x K column-major
  const double* w = nullptr; const int32_t* v = nullptr; const int32_t* u = nullptr; int64_t nnz = 0;
  int32_t traceCap = 0;
};

// does the device layer draw the probit latents in parallel (latent mode 1: set_latent_mode, latent_state, set_latent_state)?
template <class D, class = void> struct has_latent_mode : std::false_type {};
template <class D> struct has_latent_mode<D, std::void_t<decltype(&D::set_latent_mode)>> : std::true_type {};
// does the device layer offer the latent draw on its own (s4b_test_draw_latents)?  A layer without it still builds; the entry is refused there.
template <class D, class = void> struct has_test_draw_latents : std::false_type {};
template <class D> struct has_test_draw_latents<D, std::void_t<decltype(&D::test_draw_latents)>> : std::true_type {};
// does the device layer offer one evaluation of the Stan block's O(N) sums on its own (s4b_test_stan_sums)?  Likewise: refused where it is missing.
template <class D, class = void> struct has_test_stan_sums : std::false_type {};
template <class D> struct has_test_stan_sums<D, std::void_t<decltype(&D::test_stan_sums)>> : std::true_type {};

// does the device layer summarise the stored-tree predictions on the device (s4b_predict_summary)?  A layer without it still builds; the entry is refused there.
template <class D, class = void> struct has_predict_summary : std::false_type {};
template <class D> struct has_predict_summary<D, std::void_t<decltype(&D::predict_summary)>> : std::true_type {};
// one s4b_predict_summary call as the device layer sees it: host pointers, the new rows binned, the kept trees, the validated arguments
struct SummaryCall {
  const uint16_t* xb; int64_t nT; const PackedNode* nodes; size_t numNodes; const int64_t* treeStart; int64_t S; int T; const double* scale; int binary;
  int64_t maxDrawNodes;          // nodes of the largest kept draw: the route is chosen from it
  const double* offset; int M; const double* dense; const double* denseCoef; int E, q; const int32_t* ellIndex; const double* ellValue; const double* ellCoef;
  int link, G; const double* weights; int route, stageNodes, maxWorkgroups;
  double* mean; double* m2; double* average; int64_t* info;
};

// does the device layer form the partial dependence of the kept trees (s4b_partial_dependence)?  As has_predict_summary: refused where it is missing.
template <class D, class = void> struct has_partial_dependence : std::false_type {};
template <class D> struct has_partial_dependence<D, std::void_t<decltype(&D::partial_dependence)>> : std::true_type {};
// one s4b_partial_dependence call as the device layer sees it: the rows as a SummaryCall (weights: one vector or NULL = 1 / rows; mean, m2, average
// unused), the varied predictors, the grid binned as rows are, and per draw the tree order: the trees without a rule on a varied predictor in ascending
// index (numBase[k] of them), then the others in ascending index
struct PdCall {
  SummaryCall rows;
  int V, vars[2], G; const uint16_t* gridBin;          // [V x G]
  const int32_t* order; const int32_t* numBase;        // [S x T], [S]
  int64_t maxAffected, totalAffected;                  // trees with a rule on a varied predictor: the most in one draw, the sum over the draws
  double* pd;                                          // [S x G]
};

// does the device layer form per-row quantiles over the pooled kept draws of several samplers (s4b_predict_quantiles)?  As has_partial_dependence.
template <class D, class = void> struct has_predict_quantiles : std::false_type {};
template <class D> struct has_predict_quantiles<D, std::void_t<decltype(&D::predict_quantiles)>> : std::true_type {};
// one s4b_predict_quantiles call as the device layer sees it: the rows as a SummaryCall over the POOLED draws (nodes, tree starts, scales and the
// coefficient tables of the sampler and its peers concatenated, S and maxDrawNodes of the pool; weights, mean, m2, average unused)
struct QuantileCall {
  SummaryCall rows;
  int Q; const double* probs;          // [Q], each in [0, 1]
  int64_t scratchBytes;                // 0, or an upper limit on the value scratch of a chunk of rows
  double* quantiles;                   // [Q x nT], prob-major
};

// does the device layer form paired contrasts of two arms over the pooled kept draws (s4b_predict_contrast)?  As has_predict_quantiles.
template <class D, class = void> struct has_predict_contrast : std::false_type {};
template <class D> struct has_predict_contrast<D, std::void_t<decltype(&D::predict_contrast)>> : std::true_type {};
// one s4b_predict_contrast call as the device layer sees it: arm 1 as a SummaryCall over the POOLED draws (as QuantileCall.rows; weights, mean, m2,
// average in use, each NULL where it was not asked for), the D <= 2 BART columns whose bins differ in some row with arm 0's bins of them, arm 0's
// side of the linear parts that were given (NULL: arm 1's), the tree order of pd_tree_order with vars = the D columns per pooled draw, the probs
struct ContrastCall {
  SummaryCall rows;
  int D, vars[2]; const uint16_t* xb0;                 // [D x nT]
  const double* offset0; const double* dense0; const int32_t* ellIndex0; const double* ellValue0;
  const int32_t* order; const int32_t* numBase;        // [S x T], [S]
  int64_t maxAffected, totalAffected;                  // trees with a rule on a differing column: the most in one draw, the sum over the draws
  int Q; const double* probs; int64_t scratchBytes; double* quantiles;          // as QuantileCall
};

// does the device layer form per-level sums and means of the rows' values (s4b_predict_groups)?  As has_predict_contrast.
template <class D, class = void> struct has_predict_groups : std::false_type {};
template <class D> struct has_predict_groups<D, std::void_t<decltype(&D::predict_groups)>> : std::true_type {};
// one s4b_predict_groups call as the device layer sees it: the arms as a ContrastCall (one arm: its rows alone are in use, as QuantileCall.rows; no
// weights, no per-row output there), the validated non-decreasing levels, the row weights (NULL: 1), the first row of every level (levelStart[L] =
// nT) and W_l as the host formed them, the levels whose outputs are NaN, each output NULL where it was not asked for
struct GroupsCall {
  ContrastCall arms;
  int nArms; const int32_t* level; int64_t L; int statistic, hasThreshold; double threshold;
  const double* rowWeights;                            // [nT] or NULL
  const int64_t* levelStart; const double* levelWeight;          // [L + 1], [L]
  int64_t nanLevels;
  double* mean; double* m2; double* quantiles; double* pAbove; double* draws;          // [L], [L], [Q x L], [L], [L x S]
};

// does the device layer project the rows' values on a design per pooled draw (s4b_predict_projection)?  As has_predict_groups.
template <class D, class = void> struct has_predict_projection : std::false_type {};
template <class D> struct has_predict_projection<D, std::void_t<decltype(&D::predict_projection)>> : std::true_type {};
// one s4b_predict_projection call as the device layer sees it: the arms as GroupsCall's, the validated design [nT x K] row-major, the row weights
// (NULL: 1) and W > 0 as the host formed it, the pivot tolerance resolved, coef and r2 always, every other output NULL where it was not asked for
struct ProjectionCall {
  ContrastCall arms;
  int nArms; const double* design; int K;
  const double* rowWeights; double W, tol;
  int hasThreshold; double threshold;
  double* coef; double* r2;                            // [K x S], [S]
  double* mean; double* m2; double* quantiles; double* pAbove;          // [K + 1], [K + 1], [Q x (K + 1)], [K + 1]: the coefficients, then r2
};

// does the device layer form the across-row spread of the rows' values per pooled draw (s4b_predict_spread)?  As has_predict_groups.
template <class D, class = void> struct has_predict_spread : std::false_type {};
template <class D> struct has_predict_spread<D, std::void_t<decltype(&D::predict_spread)>> : std::true_type {};
// one s4b_predict_spread call as the device layer sees it: the arms as GroupsCall's, the validated thresholds [T] ascending, the row weights (NULL:
// 1), W > 0 and the slabs without weight as the host formed them, every output NULL where it was not asked for
struct SpreadCall {
  ContrastCall arms;
  int nArms; const double* thresholds; int T, binIndex;
  const double* rowWeights; double W; int64_t zeroSlabs;
  double* mean; double* m2; double* quantiles; double* draws;          // [4 + 2 T], [4 + 2 T], [Q x (4 + 2 T)], [(4 + 2 T) x S]
};

// does the device layer form the posterior predictive check per pooled draw (s4b_predict_check)?  As has_predict_spread.
template <class D, class = void> struct has_predict_check : std::false_type {};
template <class D> struct has_predict_check<D, std::void_t<decltype(&D::predict_check)>> : std::true_type {};
// one s4b_predict_check call as the device layer sees it: the rows, y, sigma per POOLED draw (link 0) and the row scale as PpdCall's, the validated
// thresholds [T] ascending, the row weights (NULL: 1), W > 0 and the slabs without weight as the host formed them; draws is always given, every
// other output NULL where it was not asked for
struct CheckCall {
  SummaryCall rows;
  const double* y; const double* sigma; const double* rowScale;          // [nT]; [S] or NULL (link 1); [nT] or NULL
  uint64_t noiseKey;
  const double* thresholds; int T, binIndex;
  const double* rowWeights; double W; int64_t zeroSlabs;
  int Q; const double* probs; int64_t scratchBytes;
  double* mean; double* m2; double* quantiles; double* draws; double* observed;          // [7 + T], [7 + T], [Q x (7 + T)], [(7 + T) x S], [5 + T]
};

// does the device layer form the per-row response curves over the pooled kept draws (s4b_predict_curves)?  As has_predict_check.
template <class D, class = void> struct has_predict_curves : std::false_type {};
template <class D> struct has_predict_curves<D, std::void_t<decltype(&D::predict_curves)>> : std::true_type {};
// one s4b_predict_curves call as the device layer sees it: the rows as QuantileCall.rows over the POOLED draws, the varied predictors, the grid binned
// as rows are and the tree order of pd_tree_order per pooled draw as PdCall's, the anchor (-1: none), every output NULL where it was not asked for
struct CurvesCall {
  SummaryCall rows;
  int V, vars[2], G, anchor; const uint16_t* gridBin;  // [V x G]
  const int32_t* order; const int32_t* numBase;        // [S x T], [S]
  int64_t maxAffected, totalAffected;
  int Q; const double* probs; int64_t scratchBytes;
  double* mean; double* m2; double* quantiles; double* pMax; double* pMin;          // [nT x G], [nT x G], [Q x nT x G], [nT x G], [nT x G]
  double* rangeMean; double* rangeM2; double* rangeQuantiles;                       // [nT], [nT], [Q x nT]
};

// does the device layer describe every row's posterior from its sorted draws (s4b_predict_describe)?  As has_predict_curves.
template <class D, class = void> struct has_predict_describe : std::false_type {};
template <class D> struct has_predict_describe<D, std::void_t<decltype(&D::predict_describe)>> : std::true_type {};
// one s4b_predict_describe call as the device layer sees it: the arms as GroupsCall's (the probs inside them), the validated window counts [nMass] and
// thresholds [nThr], every output NULL where it was not asked for (all NULL: the query, the device layer fills info with the plan and launches nothing)
struct DescribeCall {
  ContrastCall arms;
  int nArms, nMass, nThr; const int32_t* hdiCount; const double* thresholds;
  double* quantiles; double* median; double* hdi; int32_t* hdiStart;          // [Q x nT], [nT], [nMass x 2 x nT], [nMass x nT]
  int32_t* nAbove; int32_t* nBelow; double* mad;                              // [nThr x nT], [nThr x nT], [nT]
};

// does the device layer select order statistics across the rows per pooled draw (s4b_predict_sorted)?  As has_predict_describe.
template <class D, class = void> struct has_predict_sorted : std::false_type {};
template <class D> struct has_predict_sorted<D, std::void_t<decltype(&D::predict_sorted)>> : std::true_type {};
// one s4b_predict_sorted call as the device layer sees it: the arms as GroupsCall's (the probs over the draws inside them), the validated row probs
// [Qr] and cut ranks [J], every output NULL where it was not asked for (all NULL: the query, the device layer fills info with the plan and launches
// nothing)
struct SortedCall {
  ContrastCall arms;
  int nArms, Qr, J; const double* rowProbs; const int32_t* cutRank;
  double* mean; double* m2; double* quantiles; double* draws;          // [Qr + J], [Qr + J], [Q x (Qr + J)], [(Qr + J) x S]
  int32_t* nAbove; int32_t* nBelow;                                    // [J x nT] each
};
// does the device layer run the selection and count kernels alone (s4b_test_sorted_select)?  Refused where it is missing.
template <class D, class = void> struct has_test_sorted_select : std::false_type {};
template <class D> struct has_test_sorted_select<D, std::void_t<decltype(&D::test_sorted_select)>> : std::true_type {};
// one s4b_test_sorted_select call, validated: values [n x S] row-major, the ranks and the cuts, every output NULL where it was not asked for
struct SortedSelectCall {
  const double* values; int64_t n, S, blockDraws;
  int nRanks; const int32_t* ranks; double* orderStats;                // [nRanks], [nRanks x S]
  int nCuts; const int32_t* cutRank; int32_t* nAbove; int32_t* nBelow; // [nCuts], [nCuts x n] each
  int64_t* info;
};

// does the device layer form the posterior predictive read-out over the pooled kept draws (s4b_predict_ppd)?  As has_predict_quantiles.
template <class D, class = void> struct has_predict_ppd : std::false_type {};
template <class D> struct has_predict_ppd<D, std::void_t<decltype(&D::predict_ppd)>> : std::true_type {};
// one s4b_predict_ppd call as the device layer sees it: the rows as a SummaryCall over the POOLED draws (as QuantileCall.rows; link: the response, 0
// continuous, 1 binary — the value kernel writes z under either), sigma per POOLED draw (link 0), the validated arguments, each output NULL where
// it was not asked for (lmean and lm2 together)
struct PpdCall {
  SummaryCall rows;
  const double* y; const double* sigma; const double* rowScale;          // [nT] or NULL; [S] or NULL (link 1); [nT] or NULL
  uint64_t noiseKey;
  int Q; const double* probs; int64_t scratchBytes; double* quantiles;          // as QuantileCall; Q may be 0
  double* lpd; double* lmean; double* lm2; double* pit;                  // [nT] each
};

// does the device layer form the PSIS-LOO read-out over the pooled kept draws (s4b_predict_loo)?  As has_predict_ppd.
template <class D, class = void> struct has_predict_loo : std::false_type {};
template <class D> struct has_predict_loo<D, std::void_t<decltype(&D::predict_loo)>> : std::true_type {};
// one s4b_predict_loo call as the device layer sees it: the rows as PpdCall.rows (link: the response), sigma per POOLED draw (link 0), the tail
// length M resolved (the default formed, a given one checked against the pool), each output NULL where it was not asked for
struct LooCall {
  SummaryCall rows;
  const double* y; const double* sigma; const double* rowScale;          // [nT]; [S] or NULL (link 1); [nT] or NULL
  int tailLen;                                                           // M: below 5 no tail is fitted
  int64_t scratchBytes;
  double* elpd; double* khat; double* lpd; double* ess;                  // [nT] each
};

// does the device layer form split R-hat and the effective sample size per row (s4b_predict_convergence)?  As has_predict_loo.
template <class D, class = void> struct has_predict_convergence : std::false_type {};
template <class D> struct has_predict_convergence<D, std::void_t<decltype(&D::predict_convergence)>> : std::true_type {};
// one s4b_predict_convergence call as the device layer sees it: the rows as QuantileCall.rows (quantity 1: link is the response, as LooCall), the
// chains after the cut and the split as their first draws inside the pooled row and one common length, each output NULL where it was not asked for
struct ConvCall {
  SummaryCall rows;
  int quantity;                                                          // 0: the fitted value, 1: the likelihood of y
  const double* y; const double* sigma; const double* rowScale;          // quantity 1: [nT]; [S] or NULL (link 1); [nT] or NULL
  int numChains, chainLen; const int32_t* chainStart;                    // C, N, [C]
  int64_t scratchBytes;
  double* rhat; double* ess; double* mean; double* mcse; int32_t* nPairs;          // [nT] each
};

template <class Dev>
class SamplerCore {
 public:
  // stored sampler (stan4bart_createStoredBARTSampler, reference src/init.cpp:418-446): only the exported kept trees
  SamplerCore(const void* state, int64_t size, int device) {
    stored_ = true;
    Reader r{(const unsigned char*)state, (size_t)(size < 0 ? 0 : size), 0};
    if (!state || r.u32() != STATE_MAGIC) throw std::invalid_argument("not an exported stan4bart_amd BART state");
    if (r.u32() != 1u) throw std::invalid_argument("exported BART state: unknown version");
    P_ = (int)r.u32(); T_ = (int)r.u32(); binary_ = r.u32() != 0;
    const uint64_t S = r.u64(), numNodes = r.u64();
    if (P_ < 1 || P_ > 32767 || T_ < 1) throw std::invalid_argument("exported BART state: bad dimensions");
    numCuts_.resize((size_t)P_); r.get(numCuts_.data(), (size_t)P_ * 4);
    cuts_.resize((size_t)P_);
    for (int j = 0; j < P_; ++j) { if (numCuts_[(size_t)j] < 0 || numCuts_[(size_t)j] > 65534) throw std::invalid_argument("exported BART state: bad cut count");
                                   cuts_[(size_t)j].resize((size_t)numCuts_[(size_t)j]); r.get(cuts_[(size_t)j].data(), cuts_[(size_t)j].size() * 8); }
    keptScale_.resize((size_t)S * 2); r.get(keptScale_.data(), keptScale_.size() * 8);
    keptTreeStart_.resize((size_t)S * (size_t)T_); r.get(keptTreeStart_.data(), keptTreeStart_.size() * 8);
    keptNodes_.resize((size_t)numNodes); r.get(keptNodes_.data(), keptNodes_.size() * sizeof(PackedNode));
    // The byte string may come from another process (parallel.py gathers them across ranks) or from disk: nothing in it is
    // trusted.  Every tree must be a contiguous node range whose links stay inside the range and form a tree (each node reached
    // at most once from the root: no cycles, no shared children), with rules inside the cut tables — otherwise the prediction
    // kernel would read out of bounds or never terminate.
    {
      const size_t numTreesAll = keptTreeStart_.size();
      std::vector<uint8_t> seen; std::vector<int> stack;
      for (size_t k = 0; k < numTreesAll; ++k) {
        const int64_t st = keptTreeStart_[k];
        const int64_t en = k + 1 < numTreesAll ? keptTreeStart_[k + 1] : (int64_t)numNodes;
        if (st < 0 || en > (int64_t)numNodes || en <= st) throw std::invalid_argument("exported BART state: tree offset out of range");
        const int64_t count = en - st;
        if (count > 32767) throw std::invalid_argument("exported BART state: tree too large");
        const PackedNode* base = keptNodes_.data() + st;
        seen.assign((size_t)count, 0); stack.assign(1, 0);
        while (!stack.empty()) {
          const int nd = stack.back(); stack.pop_back();
          if (seen[(size_t)nd]) throw std::invalid_argument("exported BART state: node reached twice (cycle or shared child)");
          seen[(size_t)nd] = 1;
          const PackedNode& p = base[nd];
          if (p.var >= 0) {
            if (p.var >= P_) throw std::invalid_argument("exported BART state: predictor index out of range");
            if ((int)p.cut >= numCuts_[(size_t)p.var]) throw std::invalid_argument("exported BART state: cut index out of range");
            if (p.left < 0 || p.left >= count || p.right < 0 || p.right >= count) throw std::invalid_argument("exported BART state: child link out of range");
            stack.push_back(p.right); stack.push_back(p.left);
          } else if (p.var != NODE_LEAF) throw std::invalid_argument("exported BART state: unused slot linked into a tree");
        }
      }
    }
    dev_.init_stored(device, P_); groupDevice_ = device;
  }
  // stan4bart_exportBARTState (reference src/init.cpp:409-416): needed size; written when the buffer is large enough
  int64_t export_state(void* buf, int64_t cap) const {
    size_t need = 4 * 5 + 8 * 2 + (size_t)P_ * 4;
    for (int j = 0; j < P_; ++j) need += cuts_[(size_t)j].size() * 8;
    need += keptScale_.size() * 8 + keptTreeStart_.size() * 8 + keptNodes_.size() * sizeof(PackedNode);
    if (!buf || cap < (int64_t)need) return (int64_t)need;
    unsigned char* o = (unsigned char*)buf;
    auto put = [&](const void* src, size_t n) { if (n) std::memcpy(o, src, n); o += n; };
    const uint32_t head[5] = {STATE_MAGIC, 1u, (uint32_t)P_, (uint32_t)T_, binary_ ? 1u : 0u};
    const uint64_t cnt[2] = {(uint64_t)keptScale_.size() / 2, (uint64_t)keptNodes_.size()};
    put(head, sizeof(head)); put(cnt, sizeof(cnt)); put(numCuts_.data(), (size_t)P_ * 4);
    for (int j = 0; j < P_; ++j) put(cuts_[(size_t)j].data(), cuts_[(size_t)j].size() * 8);
    put(keptScale_.data(), keptScale_.size() * 8); put(keptTreeStart_.data(), keptTreeStart_.size() * 8);
    put(keptNodes_.data(), keptNodes_.size() * sizeof(PackedNode));
    return (int64_t)need;
  }

  SamplerCore(const s4b_bart_control* bc, const s4b_bart_data* bd, const s4b_stan_data* sd, const s4b_stan_control* sc,
              const s4b_common_control* cc, const uint32_t* rstate) {
    if (!bc || !bd || !sd || !sc || !cc || !rstate) throw std::invalid_argument("create: NULL argument");
    // (first thing read of the struct: a caller built against an older, shorter layout is refused before any newer field is touched)
    if (bc->interface_version != S4B_INTERFACE_VERSION) throw std::invalid_argument("s4b_bart_control.interface_version must be S4B_INTERFACE_VERSION (the caller was compiled against another revision of stan4bart_amd.h)");
    if (bd->n != sd->N) throw std::invalid_argument("bart data n != stan data N");
    if (bd->n < 1 || bd->p < 1) throw std::invalid_argument("bart data must have n >= 1, p >= 1");
    // (a rule stores its predictor as int16_t — tree arrays, PackedNode::var, with negative values for leaves and free slots: a larger index would wrap into those)
    if (bd->p > 32767) throw std::invalid_argument("bart data: at most 32767 predictors (a rule stores its predictor as int16_t)");
    if (bc->n_trees < 1) throw std::invalid_argument("n_trees must be >= 1");
    if (!(cc->sigma_init > 0)) throw std::invalid_argument("sigma_init must be > 0");
    if ((cc->is_binary != 0) != (sd->is_binary != 0)) throw std::invalid_argument("common_control.is_binary and stan_data.is_binary disagree");
    binary_ = cc->is_binary != 0;
    if (sd->has_weights) {
      if (!sd->weights) throw std::invalid_argument("has_weights = 1 but weights is NULL");
      if (cc->is_binary) throw std::invalid_argument("observation weights are not available for binary responses");
      // (+inf passes `w > 0`: the likelihood sums of both sides would turn non-finite, and the persistent sweep's weight scale with them)
      for (int64_t i = 0; i < sd->N; ++i) if (!(sd->weights[i] > 0.0) || !std::isfinite(sd->weights[i])) throw std::invalid_argument("weights must be positive and finite");
      weights_.assign(sd->weights, sd->weights + sd->N);
    }
    if (sd->has_intercept) throw std::invalid_argument("has_intercept = 1 is not supported (BART supplies the intercept)");
    if (sd->prior_dist < 0 || sd->prior_dist > 7) throw std::invalid_argument("prior_dist must be in 0..7");
    if ((sd->prior_dist == 3 || sd->prior_dist == 4) && cc->is_binary) throw std::invalid_argument("hs priors scale with the residual sd: not available for binary responses");
    if (sd->prior_dist == 7 && !sd->num_normals) throw std::invalid_argument("product_normal needs num_normals");
    n_ = (size_t)bd->n; P_ = bd->p; T_ = bc->n_trees; nTest_ = (size_t)bd->n_test;
    warmup_ = cc->warmup; verbose_ = cc->verbose; refresh_ = cc->refresh; keepFits_ = cc->keep_fits != 0; offsetType_ = cc->offset_type;
    callback_ = cc->callback; callbackUser_ = cc->callback_user;
    thin_ = bc->n_thin > 0 ? bc->n_thin : 1;
    keepTrees_ = bc->keep_trees != 0;
    nc_ = bc->node_capacity > 0 ? bc->node_capacity : 256;
    if (nc_ < 3 || nc_ > 32000) throw std::invalid_argument("node_capacity must be in [3, 32000]");
    if (cc->offset) { userOffset_.assign(cc->offset, cc->offset + n_); hasUserOffset_ = true; }
    rng_.mti = (int32_t)rstate[0]; rng_.pad = 0;
    std::memcpy(rng_.mt, rstate + 1, 624 * sizeof(uint32_t));
    latKey_ = latent_key(rstate, sc->seed);

    // ---- Stan spec + host copies of the design (the reference copies them too: stan_sampler.cpp:197-249)
    StanSpec sp;
    sp.N = sd->N; sp.K = sd->K; sp.q = sd->q; sp.t = sd->t; sp.len_theta_L = sd->len_theta_L;
    sp.is_binary = binary_ ? 1 : 0; sp.prior_dist = sd->prior_dist; sp.prior_dist_for_aux = sd->prior_dist_for_aux;
    if (sd->K) { sp.prior_scale.assign(sd->prior_scale, sd->prior_scale + sd->K); sp.prior_mean.assign(sd->prior_mean, sd->prior_mean + sd->K);
                 sp.prior_df.assign(sd->prior_df, sd->prior_df + sd->K); }
    sp.prior_scale_for_aux = sd->prior_scale_for_aux; sp.prior_mean_for_aux = sd->prior_mean_for_aux; sp.prior_df_for_aux = sd->prior_df_for_aux;
    sp.global_prior_df = sd->global_prior_df; sp.global_prior_scale = sd->global_prior_scale; sp.slab_df = sd->slab_df; sp.slab_scale = sd->slab_scale;
    if (sd->prior_dist == 7) sp.num_normals.assign(sd->num_normals, sd->num_normals + sd->K);
    if (sd->t) { sp.p.assign(sd->p, sd->p + sd->t); sp.l.assign(sd->l, sd->l + sd->t); sp.shape.assign(sd->shape, sd->shape + sd->t);
                 sp.scale.assign(sd->scale, sd->scale + sd->t); }
    if (sd->len_concentration) sp.concentration.assign(sd->concentration, sd->concentration + sd->len_concentration);
    if (sd->len_regularization) sp.regularization.assign(sd->regularization, sd->regularization + sd->len_regularization);
    {
      int qq = 0; for (int i = 0; i < sd->t; ++i) qq += sd->p[i] * sd->l[i];
      if (qq != sd->q) throw std::invalid_argument("q != sum(p * l)");
      for (int64_t e = 0; e < sd->num_non_zero; ++e) if (sd->v[e] < 0 || sd->v[e] >= sd->q) throw std::invalid_argument("CSR column index out of range");
    }
    model_.reset(new HostModel(sp));
    // test hook (tests/test_priors.py): 1 = reverse-mode tape for every gradient, 2 = closed form AND tape, compared on every evaluation
    if (const char* e = std::getenv("S4B_GRADIENT_CHECK")) model_->gradientCheck = std::atoi(e);
    K_ = sd->K; q_ = sd->q; hmcMode_ = sc->hmc_mode;
    cX_.assign((size_t)K_, 0.0); cZ_.assign((size_t)q_, 0.0);

    // ---- BART data: cut points + binning on the host (one-off), model constants
    numCuts_.assign(bd->n_cuts, bd->n_cuts + P_);
    for (int j = 0; j < P_; ++j) if (numCuts_[(size_t)j] < 0 || numCuts_[(size_t)j] > 65534) throw std::invalid_argument("n_cuts must be in [0, 65534]");
    make_cuts(bd->x, bc->use_quantiles != 0);
    std::vector<uint16_t> xbin((size_t)P_ * n_), xbinTest((size_t)P_ * nTest_);
    bin_matrix(bd->x, n_, xbin);
    if (nTest_) bin_matrix(bd->x_test, nTest_, xbinTest);

    DevInit di;
    di.n = (int64_t)n_; di.nTest = (int64_t)nTest_; di.P = P_; di.T = T_; di.nc = nc_; di.device = cc->device; groupDevice_ = cc->device;
    di.xbin = xbin.data(); di.xbinTest = nTest_ ? xbinTest.data() : nullptr; di.numCuts = numCuts_.data();
    di.y = sd->y; di.userOffset = hasUserOffset_ ? userOffset_.data() : nullptr; di.weights = weights_.empty() ? nullptr : weights_.data();
    di.model.P = P_; di.model.Pvalid = 0;
    for (int j = 0; j < P_; ++j) if (numCuts_[(size_t)j] > 0) ++di.model.Pvalid;
    if (di.model.Pvalid == 0) throw std::invalid_argument("no predictor has a cut point");
    di.model.numCuts = nullptr; di.model.scratch = nullptr; di.model.splitProbs = nullptr;
    if (bc->split_probs) {   // cgm(split.probs = ): one positive weight per predictor (reference R/stan4bart_fit.R:466-475)
      splitProbs_.assign(bc->split_probs, bc->split_probs + P_);
      for (double w : splitProbs_) if (!(w > 0.0) || !std::isfinite(w)) throw std::invalid_argument("split_probs must be positive and finite");
      di.model.splitProbs = splitProbs_.data();
    }
    di.model.base = bc->base; di.model.power = bc->power;
    di.model.pBD = bc->birth_or_death_prob; di.model.pSwap = bc->swap_prob; di.model.pChange = bc->change_prob; di.model.pBirth = bc->birth_prob;
    if (!(bc->k > 0.0) || !std::isfinite(bc->k)) throw std::invalid_argument("k must be positive and finite");
    kModeled_ = bc->k_hyper_df > 0.0; kFixed_ = bc->k;
    if (kModeled_ && !(bc->k_hyper_scale > 0.0)) throw std::invalid_argument("k_hyper_scale must be positive (or +Inf)");
    if (kModeled_ && !std::isfinite(bc->k_hyper_df)) throw std::invalid_argument("k_hyper_df must be finite");
    di.model.leafPrec = leaf_precision(bc->k, T_, bc->node_scale);
    {   // lookup tables of the tree prior, computed with the host libm (device decisions then use the same values)
      pgDepth_.resize(S4B_MAX_DEPTH); logPg_.resize(S4B_MAX_DEPTH); log1mPg_.resize(S4B_MAX_DEPTH);
      for (int d = 0; d < S4B_MAX_DEPTH; ++d) {
        pgDepth_[(size_t)d] = bc->base / std::pow(1.0 + (double)d, bc->power);
        logPg_[(size_t)d] = std::log(pgDepth_[(size_t)d]); log1mPg_[(size_t)d] = std::log(1.0 - pgDepth_[(size_t)d]);
      }
      int maxCuts = 1; for (int j = 0; j < P_; ++j) maxCuts = std::max(maxCuts, numCuts_[(size_t)j]);
      logInt_.resize((size_t)std::max(P_, maxCuts) + 2);
      for (size_t k = 0; k < logInt_.size(); ++k) logInt_[k] = std::log((double)k);
      di.model.pgDepth = pgDepth_.data(); di.model.logPg = logPg_.data(); di.model.log1mPg = log1mPg_.data();
      di.model.logInt = logInt_.data(); di.model.logIntLen = (int32_t)logInt_.size();
    }
    di.K = K_; di.q = q_; di.binary = binary_ ? 1 : 0; di.X = sd->X; di.w = sd->w; di.v = sd->v; di.u = sd->u; di.nnz = sd->num_non_zero; nnz_ = sd->num_non_zero;
    di.traceCap = 1 << 16;
    hostModelView_ = di.model; hostModelView_.numCuts = numCuts_.data();   // (table pointers are host pointers)
    dev_.init(di);
    if (kModeled_) dev_.set_k_hyper(bc->k_hyper_df, bc->k_hyper_scale, bc->node_scale, bc->k);     // normal(k = chi(df, scale)): redrawn after every sweep

    // ---- Stan sampler: init + init_stepsize run against offset_ = 0 and the raw y (reference
    //      interruptable_sampler.hpp:150,175-176 happen before any BART fit exists)
    if (hmcMode_ == 0) { build_gram(sd); haveGram_ = true; }
    dev_.stan_inputs(/*mode raw y*/ 0, false, cX_.data(), cZ_.data(), &s0_, nullptr);
    model_->lik = [this](const double* beta, const double* b, double* gX, double* gZ, double* th) { return likelihood(beta, b, gX, gZ, th); };
    NutsControl nc;
    nc.seed = sc->seed; nc.init_r = sc->init_r; nc.skip = sc->skip;
    if (nc.skip <= 0) { nc.skip = (2000 - warmup_) / 1000; if (nc.skip < 1) nc.skip = 1; }
    nc.gamma = sc->adapt_gamma; nc.delta = sc->adapt_delta; nc.kappa = sc->adapt_kappa; nc.t0 = sc->adapt_t0;
    nc.init_buffer = sc->adapt_init_buffer; nc.term_buffer = sc->adapt_term_buffer; nc.window = sc->adapt_window;
    nc.stepsize = sc->stepsize; nc.jitter = sc->stepsize_jitter; nc.max_depth = sc->max_treedepth;
    nuts_.reset(new Nuts(*model_, nc, 1, warmup_));
    // run-ahead helpers of the NUTS transition (stan_host.hpp Nuts::RunAhead): S4B_NUTS_HELPERS = 0 / 1 / 2 (more: 2, negative: 0); unset: one, and a
    // second one where the process has the cores for it (Nuts::set_helpers_auto)
    { const char* e = std::getenv("S4B_NUTS_HELPERS"); if (e && *e) { const int n = std::atoi(e); nuts_->set_helpers(n < 0 ? 0 : (n > 2 ? 2 : n)); } else nuts_->set_helpers_auto(); }
    sync_runahead();
    row_.assign((size_t)(7 + model_->sp.n_constrained), 0.0);

    // ---- BART init (reference src/init.cpp:236-273)
    std::vector<double> bartOffset(n_, 0.0);
    const double* boi = cc->bart_offset_init;
    if (hasUserOffset_) {
      if (offsetType_ != OFFSET_BART) {
        bartOffset = userOffset_;
        if (boi && offsetType_ == OFFSET_DEFAULT) for (size_t i = 0; i < n_; ++i) bartOffset[i] += boi[i];
      } else if (boi) bartOffset.assign(boi, boi + n_);
    } else if (boi) bartOffset.assign(boi, boi + n_);
    dev_.offset_from_host(bartOffset.data());
    dev_.rescale(true);
    if (!binary_) { dev_.set_sigma(cc->sigma_init); sigma_ = cc->sigma_init; } else sigma_ = 1.0;
    sample_trees_from_prior();
    dev_.sweep(thin_);
    treeUpdates_ += (long)T_ * thin_;
    dev_.stan_inputs(stan_mode(), false, cX_.data(), cZ_.data(), &s0_, nullptr);
    check_device();
  }

  // stan4bart_run (reference src/init.cpp:678-965)
  void run(int numIter, bool isWarmup, int resultsType, s4b_results* out) {
    live();
    if (numIter < 1) throw std::invalid_argument("num_iter must be >= 1");
    ran_ = true;
    dev_.reset_fused_scales();     // (history-independent at every call boundary: see DevHip::reset_fused_scales)
    const bool doStan = resultsType == 0 || resultsType == 2, doBart = resultsType == 0 || resultsType == 1;
    const int numPars = (int)row_.size();
    size_t slot = 0;
    std::vector<double> train, test;
    const bool wantTrain = (out && out->bart_train) || callback_;
    // keep_fits = FALSE keeps one result slot that every iteration overwrites (reference src/init.cpp:725-733): without a
    // callback only the last iteration's draw is observable, so nothing O(N) crosses PCIe before it
    const bool lastOnly = !keepFits_ && !callback_;
    if (wantTrain) train.resize(n_);
    if (nTest_) test.resize(nTest_);
    // reference src/init.cpp:745-747, 752-754: start line at verbose > 0, "iter k / n" every `refresh` iterations at verbose > 1.
    // With a progress hook (s4b_set_progress) the hook is called instead of printing, every `refresh` iterations (every
    // iteration when refresh <= 0), and may cancel the run by returning non-zero (the R shim polls R_CheckUserInterrupt there,
    // as the reference does per transition: src/stan_sampler.hpp:44-48)
    if (verbose_ > 0 && !progress_)
      std::printf("starting %s, %d draws, %s\n", isWarmup ? "warmup" : "sampling", numIter,
                  resultsType == 0 ? "both BART and Stan" : (resultsType == 1 ? "BART only" : "Stan only"));
    std::fflush(stdout);
    const bool timing = std::getenv("S4B_HOST_TIMING") != nullptr;
    double tph[4] = {0, 0, 0, 0};
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    for (int iter = 0; iter < numIter; ++iter) {
      if (progress_) {
        if (refresh_ <= 0 || (iter + 1) % refresh_ == 0 || iter == 0)
          if (progress_(progressUser_, iter + 1, numIter, isWarmup ? 1 : 0) != 0) throw std::runtime_error("interrupted by the progress callback");
      } else if (refresh_ > 0 && verbose_ > 1 && (iter + 1) % refresh_ == 0) { std::printf("  iter %.3d / %.3d\n", iter + 1, numIter); std::fflush(stdout); }
      double t0 = timing ? now() : 0;
      if (doStan) {
        nuts_->run(row_.data());
        if (timing) { tph[0] += now() - t0; t0 = now(); }
        const double* cons = row_.data() + 7;
        const double* beta = cons + model_->sp.beta_pos();
        const double* b = cons + model_->sp.b_pos();
        offset_by_type(beta, b);
        if (!binary_) { sigma_ = cons[model_->sp.aux_pos()]; dev_.set_sigma(sigma_); }
        if (out && out->stan) std::memcpy(out->stan + slot * (size_t)numPars, row_.data(), (size_t)numPars * sizeof(double));
        int update_scale_mod = 1 << (8 * iter / numIter);
        dev_.rescale(isWarmup && iter % update_scale_mod == 0);
        if (timing) { tph[1] += now() - t0; t0 = now(); }
      }
      if (doBart) {
        treeUpdates_ += (long)T_ * thin_;
        const bool emit = !lastOnly || iter == numIter - 1;
        if (nTest_ && emit && ((out && out->bart_test) || callback_)) dev_.request_test_fits();
        if (out && emit && out->bart_varcount) dev_.request_var_counts();
        sweep_and_stan_inputs(wantTrain && emit, (wantTrain && emit) ? train.data() : nullptr);
        if (timing) { tph[2] += now() - t0; t0 = now(); }
        if (nTest_ && emit && ((out && out->bart_test) || callback_)) dev_.test_fits(test.data());
        if (out && emit) {
          if (out->bart_sigma) out->bart_sigma[slot] = sigma_;
          if (out->bart_k) out->bart_k[slot] = kModeled_ ? dev_.k_current() : kFixed_;
          if (out->bart_train) std::memcpy(out->bart_train + slot * n_, train.data(), n_ * sizeof(double));
          if (out->bart_test && nTest_) std::memcpy(out->bart_test + slot * nTest_, test.data(), nTest_ * sizeof(double));
          if (out->bart_varcount) dev_.var_counts(out->bart_varcount + slot * (size_t)P_);
        }
        if (keepTrees_ && !isWarmup) keep_current_trees();
        // (a non-zero return stops the run after this iteration: the reference's callback is R code whose error unwinds run(),
        // src/init.cpp:855)
        if (callback_ && callback_(callbackUser_, train.data(), nTest_ ? test.data() : nullptr, row_.data(), numPars) != 0)
          throw std::runtime_error("stopped by the per-iteration callback");
        if (timing) tph[3] += now() - t0;
      }
      if (keepFits_) ++slot;
    }
    if (timing) std::fprintf(stderr, "S4B host ms/iter: nuts %.3f  offset+rescale issue %.3f  sweep + stan inputs (wait) %.3f  results %.3f\n",
                             1e3 * tph[0] / numIter, 1e3 * tph[1] / numIter, 1e3 * tph[2] / numIter, 1e3 * tph[3] / numIter);
    check_device();
  }

  // BART's offset from the parametric draw: which of X beta, Z b and the user's offset it holds is the sampler's offset type
  // (reference src/init.cpp:762-795).  The one dispatch of run() and of the hand-off test entry.
  void offset_by_type(const double* beta, const double* b) {
    if (!hasUserOffset_) { dev_.offset_from_params(beta, b, 1, 1, 0); return; }
    switch (offsetType_) {
      case OFFSET_DEFAULT: dev_.offset_from_params(beta, b, 1, 1, 1); break;
      case OFFSET_BART: dev_.offset_from_params(beta, b, 1, 1, 0); break;
      case OFFSET_RANEF: dev_.offset_from_params(beta, b, 1, 0, 1); break;
      case OFFSET_FIXEF: dev_.offset_from_params(beta, b, 0, 1, 1); break;
      case OFFSET_PARAMETRIC: dev_.offset_from_params(beta, b, 0, 0, 1); break;
    }
  }
  // TEST ENTRY (s4b_test_hand_off): what run() does between the Stan transition and the sweep, for a given (beta, b, sigma), and nothing else
  void test_hand_off(const double* beta, const double* b, double sigma, bool updateScale) {
    live();
    if ((K_ > 0 && !beta) || (q_ > 0 && !b)) throw std::invalid_argument("test_hand_off: NULL coefficients");
    for (int k = 0; k < K_; ++k) if (!std::isfinite(beta[k])) throw std::invalid_argument("test_hand_off: non-finite coefficient");
    for (int j = 0; j < q_; ++j) if (!std::isfinite(b[j])) throw std::invalid_argument("test_hand_off: non-finite coefficient");
    if (!binary_ && (!(sigma > 0.0) || !std::isfinite(sigma))) throw std::invalid_argument("test_hand_off: sigma must be positive and finite");
    offset_by_type(beta, b);
    if (!binary_) { sigma_ = sigma; dev_.set_sigma(sigma_); }
    dev_.rescale(updateScale);
    check_device();
  }

  // TEST ENTRY (s4b_test_stan_sums): one evaluation of the O(N) sums through the device layer's own stan_inputs / leapfrog_sums, into the caller's
  // buffers (cX_, cZ_, s0_ — what hmc_mode 0 evaluates from — stay)
  void test_stan_sums(int mode, const double* beta, const double* b, const int32_t* setExp, double* sums, int64_t* info) {
    live();
    if (mode < -1 || mode > 3) throw std::invalid_argument("test_stan_sums: mode must be -1 (one leapfrog's evaluation) or a Stan-offset mode 0..3");
    if (mode >= 2 && !hasUserOffset_) throw std::invalid_argument("test_stan_sums: modes 2 and 3 subtract the user's offset, this sampler has none");
    if (!sums || !info) throw std::invalid_argument("test_stan_sums: NULL output pointer");
    if (mode < 0 && ((K_ > 0 && !beta) || (q_ > 0 && !b))) throw std::invalid_argument("test_stan_sums: NULL coefficients");
    if (setExp) for (int g = 0; g < 3; ++g) if (setExp[g] < -900 || setExp[g] > 900) throw std::invalid_argument("test_stan_sums: an exponent outside [-900, 900]");
    // (a model without fixed effects or without grouping terms: the device layer wants the pointers run() hands it, which are never NULL)
    static const double none = 0.0;
    if constexpr (has_test_stan_sums<Dev>::value) { dev_.test_stan_sums(mode, beta ? beta : &none, b ? b : &none, setExp, sums, info); check_device(); }
    else throw std::invalid_argument("test_stan_sums: this device layer has no single evaluation of the Stan sums");
  }

  void disengage_adaptation() { live(); nuts_->disengage(); }
  void set_progress(s4b_progress_fn fn, void* user) { progress_ = fn; progressUser_ = user; }

  void parametric_mean(double* out) {
    live();
    const double* cons = row_.data() + 7;
    dev_.param_mean_to_host(cons + model_->sp.beta_pos(), cons + model_->sp.b_pos(), out);
  }
  void data_range(double out[2]) { live(); ScaleState s; dev_.get_scale(s); out[0] = s.min; out[1] = s.max; }
  void get_rng(uint32_t* st) { live(); dev_.download_rng(rng_); st[0] = (uint32_t)rng_.mti; std::memcpy(st + 1, rng_.mt, 624 * 4); }
  void set_rng(const uint32_t* st) { live(); rng_.mti = (int32_t)st[0]; rng_.pad = 0; std::memcpy(rng_.mt, st + 1, 624 * 4); dev_.upload_rng(rng_); }
  void dims(int64_t d[5]) { d[0] = (int64_t)row_.size(); d[1] = (int64_t)n_; d[2] = (int64_t)nTest_; d[3] = P_; d[4] = T_; }
  std::string par_names() const {
    live();
    const StanSpec& m = model_->sp;
    std::string o = "lp__\naccept_stat__\nstepsize__\ntreedepth__\nn_leapfrog__\ndivergent__\nenergy__";
    auto add = [&](const char* base, int cnt) { for (int i = 1; i <= cnt; ++i) o += "\n" + std::string(base) + "." + std::to_string(i); };
    add("z_beta", m.n_z_beta); add("global", m.hs);
    for (int k = 1; k <= (m.hs ? m.K : 0); ++k) for (int j = 1; j <= m.hs; ++j) o += "\nlocal." + std::to_string(j) + "." + std::to_string(k);
    add("caux", m.hs > 0 ? 1 : 0);
    for (int k = 1; k <= m.n_mix; ++k) o += "\nmix.1." + std::to_string(k);
    add("one_over_lambda", m.n_lambda);
    add("z_b", m.q); add("z_T", m.len_z_T); add("rho", m.len_rho); add("zeta", m.len_conc); add("tau", m.t);
    if (!m.is_binary) { add("aux_unscaled", 1); add("aux", 1); }
    add("beta", m.K); add("b", m.q); add("theta_L", m.len_theta_L);
    return o;
  }
  void print_summary() const {
    live();
    std::printf("stan4bart_amd sampler: n = %zu, p = %d, trees = %d, node capacity = %d, unconstrained stan params = %d, hmc mode = %s\n",
                n_, P_, T_, nc_, model_->sp.D, hmcMode_ == 0 ? "sufficient statistics" : "per-leapfrog kernels");
  }

  // flattened live trees, preorder (stan4bart_getTrees layout; reference src/init.cpp:583-665)
  int64_t get_trees(int64_t cap, int32_t* tree, int32_t* n_obs, int32_t* var, int32_t* split, double* value) {
    live();
    HostTrees h; download_trees(h);
    int64_t cnt = 0;
    for (int t = 0; t < T_; ++t) {
      TreeView tv = h.view(t, nc_);
      std::vector<int32_t> ncount((size_t)nc_, 0);
      { int nd, k; Walker<TreeView> w(tv, 0);   // post-order: counts of internal nodes
        while (w.next(nd, k)) { if (k == 0) ncount[(size_t)nd] = h.cnt[(size_t)t * nc_ + nd]; else if (k == 2) ncount[(size_t)nd] = ncount[(size_t)tv.left.get(nd)] + ncount[(size_t)tv.right.get(nd)]; } }
      int nd, k; Walker<TreeView> w(tv, 0);
      while (w.next(nd, k)) {
        if (k == 2) continue;
        if (cnt < cap && tree) {
          tree[cnt] = t; n_obs[cnt] = ncount[(size_t)nd];
          if (k == 1) { var[cnt] = tv.var.get(nd); split[cnt] = tv.cut.get(nd); value[cnt] = cuts_[(size_t)tv.var.get(nd)][(size_t)tv.cut.get(nd)]; }
          else { var[cnt] = -1; split[cnt] = -1; value[cnt] = h.mu[(size_t)t * nc_ + nd]; }
        }
        ++cnt;
      }
    }
    return cnt;
  }
  // stan4bart_getTrees(current = FALSE) over the kept draws (reference src/init.cpp:514-671; extract(fit, "trees", sampleNums = , treeNums = )):
  // 0-based index vectors select draws / trees (NULL = all, in order); same flattened layout as get_trees plus the draw index
  int64_t get_kept_trees_indexed(const int32_t* sampleIdx, int64_t numSamples, const int32_t* treeIdx, int64_t numTrees, int64_t cap, int32_t* smp,
                                 int32_t* tree, int32_t* n_obs, int32_t* var, int32_t* split, double* value) const {
    const int64_t S = (int64_t)keptScale_.size() / 2;
    if (sampleIdx && numSamples > S) throw std::invalid_argument(std::to_string(numSamples) + " samples specified but only " + std::to_string(S) + " in sampler");
    if (treeIdx && numTrees > T_) throw std::invalid_argument(std::to_string(numTrees) + " trees specified but only " + std::to_string(T_) + " in sampler");
    const int64_t nS = sampleIdx ? numSamples : S, nT = treeIdx ? numTrees : (int64_t)T_;
    int64_t cnt = 0;
    std::vector<int> stack;
    for (int64_t a = 0; a < nS; ++a) {
      const int64_t k = sampleIdx ? (int64_t)sampleIdx[a] : a;
      if (k < 0 || k >= S) throw std::invalid_argument("sample index out of range");
      for (int64_t b = 0; b < nT; ++b) {
        const int t = treeIdx ? (int)treeIdx[b] : (int)b;
        if (t < 0 || t >= T_) throw std::invalid_argument("tree index out of range");
        const PackedNode* base = keptNodes_.data() + keptTreeStart_[(size_t)(k * T_ + t)];
        stack.assign(1, 0);
        while (!stack.empty()) {   // preorder
          const int nd = stack.back(); stack.pop_back();
          const PackedNode& p = base[nd];
          if (cnt < cap && tree) {
            smp[cnt] = (int32_t)k; tree[cnt] = t; n_obs[cnt] = p.n;
            if (p.var >= 0) { var[cnt] = p.var; split[cnt] = p.cut; value[cnt] = cuts_[(size_t)p.var][(size_t)p.cut]; }
            else { var[cnt] = -1; split[cnt] = -1; value[cnt] = p.mu; }
          }
          ++cnt;
          if (p.var >= 0) { stack.push_back(p.right); stack.push_back(p.left); }
        }
      }
    }
    return cnt;
  }
  int64_t get_kept_trees(int64_t sample, int64_t cap, int32_t* smp, int32_t* tree, int32_t* n_obs, int32_t* var, int32_t* split, double* value) const {
    const int64_t S = (int64_t)keptScale_.size() / 2;
    if (sample >= S) throw std::invalid_argument("sample index out of range");
    if (sample < 0) return get_kept_trees_indexed(nullptr, 0, nullptr, 0, cap, smp, tree, n_obs, var, split, value);
    const int32_t one = (int32_t)sample;
    return get_kept_trees_indexed(&one, 1, nullptr, 0, cap, smp, tree, n_obs, var, split, value);
  }
  // stan4bart_printTrees (reference src/init.cpp:448-512 hands the indices to dbarts' printer, whose text format is not part of
  // the reference tree): one line per node, indented by depth — "var <= cut value [n]" for rules, "mu [n]" for leaves
  void print_trees(const int32_t* sampleIdx, int64_t numSamples, const int32_t* treeIdx, int64_t numTrees) const {
    const int64_t S = (int64_t)keptScale_.size() / 2;
    const int64_t nS = sampleIdx ? numSamples : S, nT = treeIdx ? numTrees : (int64_t)T_;
    if (sampleIdx && numSamples > S) throw std::invalid_argument(std::to_string(numSamples) + " samples specified but only " + std::to_string(S) + " in sampler");
    if (treeIdx && numTrees > T_) throw std::invalid_argument(std::to_string(numTrees) + " trees specified but only " + std::to_string(T_) + " in sampler");
    std::vector<std::pair<int, int>> stack;
    for (int64_t a = 0; a < nS; ++a) {
      const int64_t k = sampleIdx ? (int64_t)sampleIdx[a] : a;
      if (k < 0 || k >= S) throw std::invalid_argument("sample index out of range");
      for (int64_t b = 0; b < nT; ++b) {
        const int t = treeIdx ? (int)treeIdx[b] : (int)b;
        if (t < 0 || t >= T_) throw std::invalid_argument("tree index out of range");
        std::printf("sample %lld tree %d:\n", (long long)k + 1, t + 1);
        const PackedNode* base = keptNodes_.data() + keptTreeStart_[(size_t)(k * T_ + t)];
        stack.assign(1, std::make_pair(0, 0));
        while (!stack.empty()) {
          const int nd = stack.back().first, depth = stack.back().second; stack.pop_back();
          const PackedNode& p = base[nd];
          for (int d = 0; d < depth; ++d) std::printf("  ");
          if (p.var >= 0) { std::printf("x%d <= %g [n = %d]\n", p.var + 1, cuts_[(size_t)p.var][(size_t)p.cut], p.n); stack.push_back(std::make_pair((int)p.right, depth + 1)); stack.push_back(std::make_pair((int)p.left, depth + 1)); }
          else std::printf("mu = %g [n = %d]\n", p.mu, p.n);
        }
      }
    }
    std::fflush(stdout);
  }
  // stan4bart_predictBART over the trees kept while sampling (reference src/init.cpp:354-403)
  int64_t predict(const double* xTest, int64_t nT, double* out, const double* offsetTest = nullptr) {
    const int64_t S = (int64_t)keptScale_.size() / 2;
    if (!out) return S;
    if (nT < 1 || !xTest) throw std::invalid_argument("predict: x_test must have at least one row");
    if (S == 0) return 0;
    std::vector<uint16_t> xb((size_t)P_ * (size_t)nT);
    bin_matrix(xTest, (size_t)nT, xb);
    dev_.predict_stored(xb.data(), nT, keptNodes_.data(), keptNodes_.size(), keptTreeStart_.data(), S, T_, keptScale_.data(), binary_ ? 1 : 0, out);
    // offset_test of stan4bart_predictBART (reference src/init.cpp:377-384): added to every draw's prediction
    if (offsetTest) for (int64_t k = 0; k < S; ++k) for (int64_t i = 0; i < nT; ++i) out[(size_t)k * (size_t)nT + (size_t)i] += offsetTest[i];
    return S;
  }
  // s4b_predict_summary: per-row mean / m2 over the kept draws and per-draw weighted row sums of bart + offset + dense + ELL parts (link 0 / 1),
  // formed on the device without the [rows x draws] matrix.  Everything is validated here, before any launch.  Live (kept trees) and stored samplers.
  int64_t predict_summary(const s4b_summary_in* in, s4b_summary_out* out) {
    if (!out) throw std::invalid_argument("predict_summary: NULL output struct");
    for (int j = 0; j < 8; ++j) out->info[j] = 0;
    const int64_t S = (int64_t)keptScale_.size() / 2;
    out->num_samples = S;
    if (!in || (!out->mean && !out->m2 && !out->average)) return S;          // query
    if constexpr (has_predict_summary<Dev>::value) {
      const int64_t nT = in->n_test;
      check_summary_rows(in, "predict_summary", 8);
      if (!out->mean || !out->m2 || (in->n_weights > 0 && !out->average)) throw std::invalid_argument("predict_summary: mean, m2 and (with weights) average must all be given");
      if (S == 0) throw std::invalid_argument("predict_summary: the sampler holds no kept draws (bart_control.keep_trees, sampling runs)");
      std::vector<uint16_t> xb((size_t)P_ * (size_t)nT);
      bin_matrix(in->x_test, (size_t)nT, xb);
      SummaryCall c = summary_call(in, xb, S);
      c.mean = out->mean; c.m2 = out->m2; c.average = out->average; c.info = out->info;
      dev_.predict_summary(c);
      return S;
    } else throw std::invalid_argument("predict_summary: this device layer has no summary kernel (the summaries are formed by the HIP library only)");
  }
  // per draw the tree order of a partial-dependence call: the trees without a rule on vars[0 .. V) in ascending index, then the others in ascending
  // index; numBase[k] = size of the first group.  One pass over keptNodes_ (slots that a tree has given up carry NODE_FREE: no rule).
  void pd_tree_order(int V, const int32_t* vars, std::vector<int32_t>& order, std::vector<int32_t>& numBase, int64_t& maxAffected, int64_t& totalAffected) const {
    const int64_t S = (int64_t)keptScale_.size() / 2;
    order.resize((size_t)(S * T_)); numBase.resize((size_t)S); maxAffected = totalAffected = 0;
    std::vector<int32_t> affected;
    for (int64_t k = 0; k < S; ++k) {
      affected.clear();
      int32_t* o = order.data() + (size_t)(k * T_); int32_t nb = 0;
      for (int t = 0; t < T_; ++t) {
        const size_t x = (size_t)(k * T_ + t);
        const int64_t en = x + 1 < keptTreeStart_.size() ? keptTreeStart_[x + 1] : (int64_t)keptNodes_.size();
        bool hit = false;
        for (int64_t u = keptTreeStart_[x]; u < en && !hit; ++u) { const int16_t v = keptNodes_[(size_t)u].var; hit = v >= 0 && (v == vars[0] || (V > 1 && v == vars[1])); }
        if (hit) affected.push_back(t); else o[nb++] = t;
      }
      std::copy(affected.begin(), affected.end(), o + nb);
      numBase[(size_t)k] = nb;
      maxAffected = std::max<int64_t>(maxAffected, (int64_t)affected.size()); totalAffected += (int64_t)affected.size();
    }
  }
  // s4b_partial_dependence: per kept draw and grid point the weighted row sum of the prediction with the predictors `vars` set to the grid point's
  // values (the linear parts at the rows' own values), in one fused device call.  Everything is validated here, before any launch.  Live and stored samplers.
  int64_t partial_dependence(const s4b_pd_in* in, s4b_pd_out* out) {
    if (!out) throw std::invalid_argument("partial_dependence: NULL output struct");
    for (int j = 0; j < 8; ++j) out->info[j] = 0;
    const int64_t S = (int64_t)keptScale_.size() / 2;
    out->num_samples = S;
    if (!in || !out->pd) return S;          // query
    if constexpr (has_partial_dependence<Dev>::value) {
      const std::string who = "partial_dependence";
      check_summary_rows(&in->rows, who, 1);
      if (in->n_vars != 1 && in->n_vars != 2) throw std::invalid_argument(who + ": one or two varied predictors, not " + std::to_string(in->n_vars));
      for (int w = 0; w < in->n_vars; ++w)
        if (in->vars[w] < 0 || in->vars[w] >= P_) throw std::invalid_argument(who + ": predictor " + std::to_string(in->vars[w]) + " outside [0, " + std::to_string(P_) + ")");
      if (in->n_vars == 2 && in->vars[0] == in->vars[1]) throw std::invalid_argument(who + ": the two varied predictors must differ");
      if (in->n_grid < 1 || in->n_grid > 64) throw std::invalid_argument(who + ": between 1 and 64 grid points per call, not " + std::to_string(in->n_grid));
      if (!in->grid) throw std::invalid_argument(who + ": NULL grid");
      const int V = in->n_vars, G = in->n_grid;
      for (int x = 0; x < V * G; ++x) if (std::isnan(in->grid[x])) throw std::invalid_argument(who + ": the grid holds a NaN");
      if (S == 0) throw std::invalid_argument(who + ": the sampler holds no kept draws (bart_control.keep_trees, sampling runs)");
      const int64_t nT = in->rows.n_test;
      std::vector<uint16_t> xb((size_t)P_ * (size_t)nT);
      bin_matrix(in->rows.x_test, (size_t)nT, xb);
      std::vector<uint16_t> gridBin((size_t)(V * G));          // bin_matrix's rule: the number of cuts strictly below the value
      for (int w = 0; w < V; ++w) {
        const std::vector<double>& c = cuts_[(size_t)in->vars[w]];
        for (int g = 0; g < G; ++g) gridBin[(size_t)(w * G + g)] = (uint16_t)(std::lower_bound(c.begin(), c.end(), in->grid[w * G + g]) - c.begin());
      }
      PdCall c{};
      c.rows = summary_call(&in->rows, xb, S); c.rows.info = out->info;
      c.V = V; c.vars[0] = in->vars[0]; c.vars[1] = V > 1 ? in->vars[1] : -1; c.G = G; c.gridBin = gridBin.data(); c.pd = out->pd;
      std::vector<int32_t> order, numBase;
      pd_tree_order(V, in->vars, order, numBase, c.maxAffected, c.totalAffected);
      c.order = order.data(); c.numBase = numBase.data();
      dev_.partial_dependence(c);
      return S;
    } else throw std::invalid_argument("partial_dependence: this device layer has no partial-dependence kernel (it is formed by the HIP library only)");
  }
  // s4b_predict_quantiles: per row the type-7 quantiles of predict_summary's value over the kept draws of this sampler and of `peers` (n_peers of
  // them, in this order behind its own), in one device call that sees all of them.  The rows are binned once, with this sampler's cut points, so a
  // peer must carry the same predictors, trees per draw, response kind and bit-identical cut points.  Everything is validated here, before any launch.
  int64_t predict_quantiles(const s4b_quantile_in* in, s4b_quantile_out* out, const SamplerCore* const* peers) {
    if (!out) throw std::invalid_argument("predict_quantiles: NULL output struct");
    for (int j = 0; j < 8; ++j) out->info[j] = 0;
    const int64_t own = (int64_t)keptScale_.size() / 2;
    out->num_samples = own;
    if (!in || !out->quantiles) return own;          // query
    if constexpr (has_predict_quantiles<Dev>::value) {
      const std::string who = "predict_quantiles";
      const s4b_summary_in* rw = &in->rows;
      check_summary_rows(rw, who, 8);
      if (rw->n_weights != 0) throw std::invalid_argument(who + ": n_weights must be 0 (the quantiles are per row), not " + std::to_string(rw->n_weights));
      if (in->n_probs < 1 || in->n_probs > 16) throw std::invalid_argument(who + ": between 1 and 16 probs per call, not " + std::to_string(in->n_probs));
      if (!in->probs) throw std::invalid_argument(who + ": NULL probs");
      for (int j = 0; j < in->n_probs; ++j)
        if (!(in->probs[j] >= 0.0 && in->probs[j] <= 1.0)) throw std::invalid_argument(who + ": prob " + std::to_string(in->probs[j]) + " outside [0, 1]");
      if (in->scratch_bytes < 0) throw std::invalid_argument(who + ": negative scratch_bytes");
      const int np = in->n_peers;
      const int64_t S = pool_check(who, rw, np, in->peers != nullptr, peers, in->peer_dense_coef, in->peer_ell_coef);
      const int64_t nT = rw->n_test;
      std::vector<uint16_t> xb((size_t)P_ * (size_t)nT);
      bin_matrix(rw->x_test, (size_t)nT, xb);
      QuantileCall c{};
      c.rows = summary_call(rw, xb, own); c.rows.info = out->info; c.rows.G = 0; c.rows.weights = nullptr;
      c.Q = in->n_probs; c.probs = in->probs; c.scratchBytes = in->scratch_bytes; c.quantiles = out->quantiles;
      DrawPool pool;
      pool_concat(c.rows, pool, rw, xb, np, peers, in->peer_dense_coef, in->peer_ell_coef, S);
      dev_.predict_quantiles(c);
      out->num_samples = S;
      return S;
    } else throw std::invalid_argument("predict_quantiles: this device layer has no quantile kernels (the quantiles are formed by the HIP library only)");
  }
  // s4b_predict_contrast: the paired contrast d(i,k) = v(z_1) - v(z_0) of two arms over the same rows and the same pooled draws, summarised on the
  // device (mean, m2 and quantiles per row, weighted row sums per draw).  The arms are binned with this sampler's cut points; the BART columns whose
  // BINS differ in some row (at most two) are the only ones of arm 0 that travel.  Pooled like predict_quantiles.  Everything is validated here,
  // before any launch.
  int64_t predict_contrast(const s4b_contrast_in* in, s4b_contrast_out* out, const SamplerCore* const* peers) {
    if (!out) throw std::invalid_argument("predict_contrast: NULL output struct");
    for (int j = 0; j < 8; ++j) out->info[j] = 0;
    const int64_t own = (int64_t)keptScale_.size() / 2;
    out->num_samples = own;
    if (!in || (!out->mean && !out->m2 && !out->average && !out->quantiles)) return own;          // query
    if constexpr (has_predict_contrast<Dev>::value) {
      const std::string who = "predict_contrast";
      const s4b_summary_in* rw = &in->rows;
      contrast_check_in(who, in, 8);
      if ((out->mean == nullptr) != (out->m2 == nullptr)) throw std::invalid_argument(who + ": mean and m2 are given together or not at all");
      if (rw->n_weights > 0 && !out->average) throw std::invalid_argument(who + ": n_weights > 0 needs average");
      if (in->n_probs > 0 && !out->quantiles) throw std::invalid_argument(who + ": n_probs > 0 needs quantiles");
      if (!out->mean && rw->n_weights == 0 && in->n_probs == 0) throw std::invalid_argument(who + ": nothing asked for (no per-row output, no weights, no probs)");
      ContrastCall c{};
      ArmsHold hold;
      const int64_t S = contrast_arms(who, in, peers, true, out->info, c, hold);
      c.rows.mean = out->mean; c.rows.m2 = out->m2; c.rows.average = out->average; c.quantiles = out->quantiles;
      dev_.predict_contrast(c);
      out->num_samples = S;
      return S;
    } else throw std::invalid_argument("predict_contrast: this device layer has no contrast kernels (the contrasts are formed by the HIP library only)");
  }
  // s4b_predict_groups: per level of a non-decreasing row labelling the weighted sum or mean of the rows' values per pooled draw — one arm:
  // predict_quantiles' value, two arms: predict_contrast's d — and of that level series the mean, m2, type-7 quantiles and the share of the draws above
  // a threshold.  W_l and the counts are formed here, in row order.  Everything is validated here, before any launch.
  int64_t predict_groups(const s4b_groups_in* in, s4b_groups_out* out, const SamplerCore* const* peers) {
    if (!out) throw std::invalid_argument("predict_groups: NULL output struct");
    for (int j = 0; j < 8; ++j) out->info[j] = 0;
    const int64_t own = (int64_t)keptScale_.size() / 2;
    out->num_samples = own;
    if (!in || (!out->mean && !out->m2 && !out->quantiles && !out->p_above && !out->weight && !out->count && !out->draws)) return own;          // query
    if constexpr (has_predict_groups<Dev>::value) {
      const std::string who = "predict_groups";
      const s4b_contrast_in* ar = &in->arms;
      const s4b_summary_in* rw = &ar->rows;
      contrast_check_in(who, ar, 1);
      if (in->n_arms != 1 && in->n_arms != 2) throw std::invalid_argument(who + ": n_arms must be 1 (the fitted value) or 2 (the contrast), not " + std::to_string(in->n_arms));
      if (in->n_arms == 1 && (ar->x_test0 || ar->offset0 || ar->dense0 || ar->ell_index0 || ar->ell_value0))
        throw std::invalid_argument(who + ": n_arms = 1 takes no arm-0 pointer (x_test0, offset0, dense0, ell_index0, ell_value0 must be NULL)");
      if (in->statistic != 0 && in->statistic != 1) throw std::invalid_argument(who + ": statistic must be 0 (the sum) or 1 (the mean), not " + std::to_string(in->statistic));
      if (in->has_threshold != 0 && in->has_threshold != 1) throw std::invalid_argument(who + ": has_threshold must be 0 or 1");
      if (in->has_threshold && std::isnan(in->threshold)) throw std::invalid_argument(who + ": the threshold is a NaN");
      if (out->p_above && !in->has_threshold) throw std::invalid_argument(who + ": p_above needs a threshold");
      if (ar->n_probs > 0 && !out->quantiles) throw std::invalid_argument(who + ": n_probs > 0 needs quantiles");
      if (!in->level) throw std::invalid_argument(who + ": NULL level");
      if (in->n_levels < 1 || in->n_levels > 2147483647) throw std::invalid_argument(who + ": n_levels must lie in [1, 2^31), not " + std::to_string(in->n_levels));
      if (in->level_bytes < 0) throw std::invalid_argument(who + ": negative level_bytes");
      const int64_t nT = rw->n_test, L = in->n_levels;
      for (int64_t i = 0; i < nT; ++i) {
        const int64_t l = in->level[i];
        if (l < 0 || l >= L) throw std::invalid_argument(who + ": level " + std::to_string(l) + " of row " + std::to_string(i) + " outside [0, " + std::to_string(L) + ")");
        if (i > 0 && l < in->level[i - 1]) throw std::invalid_argument(who + ": the levels decrease at row " + std::to_string(i) + " (the rows of a level are contiguous: sort the rows by level, stably)");
      }
      if (rw->n_weights)
        for (int64_t i = 0; i < nT; ++i)
          if (!(rw->weights[i] >= 0.0) || std::isinf(rw->weights[i])) throw std::invalid_argument(who + ": weight " + std::to_string(rw->weights[i]) + " of row " + std::to_string(i) + " is negative or not finite");
      GroupsCall g{};
      ArmsHold hold;
      const int64_t S = contrast_arms(who, ar, peers, in->n_arms == 2, nullptr, g.arms, hold);
      const int64_t limit = in->level_bytes > 0 ? std::min<int64_t>(in->level_bytes, S4B_GROUPS_LEVEL_BYTES_MAX) : S4B_GROUPS_LEVEL_BYTES_MAX;
      if (L > limit / (8 * S))
        throw std::invalid_argument(who + ": the level matrix of " + std::to_string(L) + " levels x " + std::to_string(S) + " pooled draws exceeds " + std::to_string(limit) + " bytes (split the levels into consecutive ranges, one call each)");
      // the first row of every level, W_l and the counts: in row order, in double
      std::vector<int64_t> start((size_t)L + 1, nT);
      std::vector<double> W((size_t)L, 0.0);
      for (int64_t i = nT - 1; i >= 0; --i) start[(size_t)in->level[i]] = i;
      for (int64_t l = L - 1; l >= 0; --l) if (start[(size_t)l] > start[(size_t)l + 1]) start[(size_t)l] = start[(size_t)l + 1];          // (a level without rows starts where the next one does)
      for (int64_t i = 0; i < nT; ++i) W[(size_t)in->level[i]] += rw->n_weights ? rw->weights[i] : 1.0;
      for (int64_t l = 0; l < L; ++l) {
        const int64_t n = start[(size_t)l + 1] - start[(size_t)l];
        if (n == 0 || (in->statistic == 1 && W[(size_t)l] == 0.0)) ++g.nanLevels;
        if (out->weight) out->weight[l] = W[(size_t)l];
        if (out->count) out->count[l] = n;
      }
      g.arms.rows.info = out->info; g.arms.rows.G = 0; g.arms.rows.weights = nullptr;
      g.nArms = in->n_arms; g.level = in->level; g.L = L; g.statistic = in->statistic; g.hasThreshold = in->has_threshold; g.threshold = in->threshold;
      g.rowWeights = rw->n_weights ? rw->weights : nullptr; g.levelStart = start.data(); g.levelWeight = W.data();
      g.mean = out->mean; g.m2 = out->m2; g.quantiles = ar->n_probs > 0 ? out->quantiles : nullptr; g.pAbove = out->p_above; g.draws = out->draws;
      dev_.predict_groups(g);
      out->num_samples = S;
      return S;
    } else throw std::invalid_argument("predict_groups: this device layer has no level kernels (the per-level read-out is formed by the HIP library only)");
  }
  // s4b_predict_projection: per pooled draw the weighted least-squares coefficients of the rows' values — one arm: predict_quantiles' value, two arms:
  // predict_contrast's d — on a design of at most 32 columns, the share of the variation the projection captures, and of those series the mean, m2,
  // type-7 quantiles and the share of the draws above a threshold.  W is formed here, in row order.  Everything is validated here, before any launch.
  int64_t predict_projection(const s4b_projection_in* in, s4b_projection_out* out, const SamplerCore* const* peers) {
    if (!out) throw std::invalid_argument("predict_projection: NULL output struct");
    for (int j = 0; j < 8; ++j) out->info[j] = 0;
    out->weight = 0.0;
    const int64_t own = (int64_t)keptScale_.size() / 2;
    out->num_samples = own;
    if (!in || (!out->coef && !out->r2 && !out->mean && !out->m2 && !out->quantiles && !out->p_above)) return own;          // query
    if constexpr (has_predict_projection<Dev>::value) {
      const std::string who = "predict_projection";
      const s4b_contrast_in* ar = &in->arms;
      const s4b_summary_in* rw = &ar->rows;
      const int64_t nT = rw->n_test;
      const int K = in->n_columns;
      if (!out->coef || !out->r2) throw std::invalid_argument(who + ": coef and r2 are always returned (NULL pointer)");
      if (K < 1 || K > S4B_PROJECTION_COLUMNS_MAX)
        throw std::invalid_argument(who + ": n_columns must lie in [1, " + std::to_string(S4B_PROJECTION_COLUMNS_MAX) + "], not " + std::to_string(K));
      if (in->n_arms != 1 && in->n_arms != 2) throw std::invalid_argument(who + ": n_arms must be 1 (the fitted value) or 2 (the contrast), not " + std::to_string(in->n_arms));
      if (in->has_threshold != 0 && in->has_threshold != 1) throw std::invalid_argument(who + ": has_threshold must be 0 or 1");
      if (in->has_threshold && std::isnan(in->threshold)) throw std::invalid_argument(who + ": the threshold is a NaN");
      if (out->p_above && !in->has_threshold) throw std::invalid_argument(who + ": p_above needs a threshold");
      if (!(in->tol >= 0.0 && in->tol < 1.0)) throw std::invalid_argument(who + ": tol must lie in [0, 1) (0: the default 1e-10), not " + std::to_string(in->tol));
      if (nT < 0) throw std::invalid_argument(who + ": negative n_test");
      // what answers NaN in every floating output without a launch: `why` goes to info[6]
      auto unanswered = [&](int64_t S, int64_t why) {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        const size_t L = (size_t)K + 1, Q = (size_t)std::max(0, ar->n_probs);
        std::fill(out->coef, out->coef + (size_t)K * (size_t)S, nan); std::fill(out->r2, out->r2 + S, nan);
        if (out->mean) std::fill(out->mean, out->mean + L, nan);
        if (out->m2) std::fill(out->m2, out->m2 + L, nan);
        if (out->p_above) std::fill(out->p_above, out->p_above + L, nan);
        if (out->quantiles) std::fill(out->quantiles, out->quantiles + Q * L, nan);
        out->info[5] = S; out->info[6] = why; out->info[7] = K; out->num_samples = S;
        return S;
      };
      if (nT == 0) {          // no rows: nothing to project
        if (ar->n_probs < 0 || ar->n_probs > 16) throw std::invalid_argument(who + ": between 0 and 16 probs per call, not " + std::to_string(ar->n_probs));
        return unanswered(pool_check(who, rw, ar->n_peers, ar->peers != nullptr, peers, ar->peer_dense_coef, ar->peer_ell_coef), 3);
      }
      contrast_check_in(who, ar, 1);
      if (in->n_arms == 1 && (ar->x_test0 || ar->offset0 || ar->dense0 || ar->ell_index0 || ar->ell_value0))
        throw std::invalid_argument(who + ": n_arms = 1 takes no arm-0 pointer (x_test0, offset0, dense0, ell_index0, ell_value0 must be NULL)");
      if (ar->n_probs > 0 && !out->quantiles) throw std::invalid_argument(who + ": n_probs > 0 needs quantiles");
      if (!in->design) throw std::invalid_argument(who + ": NULL design");
      if ((int64_t)K > nT) throw std::invalid_argument(who + ": " + std::to_string(K) + " design columns, but only " + std::to_string(nT) + " rows");
      for (int64_t i = 0; i < nT; ++i)
        for (int j = 0; j < K; ++j)
          if (!std::isfinite(in->design[(size_t)i * (size_t)K + (size_t)j]))
            throw std::invalid_argument(who + ": design entry (" + std::to_string(i) + ", " + std::to_string(j) + ") is not finite");
      double W = 0.0;          // in row order, in double: part of the definition
      for (int64_t i = 0; i < nT; ++i) {
        const double w = rw->n_weights ? rw->weights[i] : 1.0;
        if (!(w >= 0.0) || std::isinf(w)) throw std::invalid_argument(who + ": weight " + std::to_string(w) + " of row " + std::to_string(i) + " is negative or not finite");
        W += w;
      }
      out->weight = W;
      ProjectionCall g{};
      ArmsHold hold;
      const int64_t S = contrast_arms(who, ar, peers, in->n_arms == 2, nullptr, g.arms, hold);
      if (W == 0.0) return unanswered(S, 2);
      g.arms.rows.info = out->info; g.arms.rows.G = 0; g.arms.rows.weights = nullptr;
      g.nArms = in->n_arms; g.design = in->design; g.K = K; g.rowWeights = rw->n_weights ? rw->weights : nullptr; g.W = W;
      g.tol = in->tol > 0.0 ? in->tol : 1e-10; g.hasThreshold = in->has_threshold; g.threshold = in->threshold;
      g.coef = out->coef; g.r2 = out->r2; g.mean = out->mean; g.m2 = out->m2; g.quantiles = ar->n_probs > 0 ? out->quantiles : nullptr; g.pAbove = out->p_above;
      dev_.predict_projection(g);
      out->num_samples = S;
      return S;
    } else throw std::invalid_argument("predict_projection: this device layer has no projection kernels (the per-draw least squares is formed by the HIP library only)");
  }
  // s4b_predict_spread: per pooled draw the weighted mean, standard deviation and extremes of the rows' values ACROSS THE ROWS — one arm:
  // predict_quantiles' value, two arms: predict_contrast's d — and the share of the weight, and the part of the mean, above each of up to 64
  // thresholds; of those series the mean, m2 and type-7 quantiles over the draws.  W and the slabs without weight are formed here, in row order.
  // Everything is validated here, before any launch.
  int64_t predict_spread(const s4b_spread_in* in, s4b_spread_out* out, const SamplerCore* const* peers) {
    if (!out) throw std::invalid_argument("predict_spread: NULL output struct");
    for (int j = 0; j < 8; ++j) out->info[j] = 0;
    out->weight = 0.0;
    const int64_t own = (int64_t)keptScale_.size() / 2;
    out->num_samples = own;
    if (!in || (!out->mean && !out->m2 && !out->quantiles && !out->draws)) return own;          // query
    if constexpr (has_predict_spread<Dev>::value) {
      const std::string who = "predict_spread";
      const s4b_contrast_in* ar = &in->arms;
      const s4b_summary_in* rw = &ar->rows;
      const int T = in->n_thresholds;
      if (T < 0 || T > S4B_SPREAD_THRESHOLDS_MAX)
        throw std::invalid_argument(who + ": n_thresholds must lie in [0, " + std::to_string(S4B_SPREAD_THRESHOLDS_MAX) + "], not " + std::to_string(T));
      if (T > 0 && !in->thresholds) throw std::invalid_argument(who + ": NULL thresholds");
      for (int j = 0; j < T; ++j) {
        if (std::isnan(in->thresholds[j])) throw std::invalid_argument(who + ": threshold " + std::to_string(j) + " is a NaN");
        if (j > 0 && !(in->thresholds[j] > in->thresholds[j - 1])) throw std::invalid_argument(who + ": the thresholds are not strictly ascending at index " + std::to_string(j));
      }
      if (in->n_arms != 1 && in->n_arms != 2) throw std::invalid_argument(who + ": n_arms must be 1 (the fitted value) or 2 (the contrast), not " + std::to_string(in->n_arms));
      if (in->bin_index < 0 || in->bin_index > 2) throw std::invalid_argument(who + ": bin_index must be 0 (the library's choice), 1 (compares) or 2 (search), not " + std::to_string(in->bin_index));
      contrast_check_in(who, ar, 1);
      if (in->n_arms == 1 && (ar->x_test0 || ar->offset0 || ar->dense0 || ar->ell_index0 || ar->ell_value0))
        throw std::invalid_argument(who + ": n_arms = 1 takes no arm-0 pointer (x_test0, offset0, dense0, ell_index0, ell_value0 must be NULL)");
      if (ar->n_probs > 0 && !out->quantiles) throw std::invalid_argument(who + ": n_probs > 0 needs quantiles");
      const int64_t nT = rw->n_test;
      double W = 0.0, Ws = 0.0;          // in row order, in double: part of the definition
      int64_t zeroSlabs = 0;
      for (int64_t i = 0; i < nT; ++i) {
        const double w = rw->n_weights ? rw->weights[i] : 1.0;
        if (!(w >= 0.0) || std::isinf(w)) throw std::invalid_argument(who + ": weight " + std::to_string(w) + " of row " + std::to_string(i) + " is negative or not finite");
        W += w; Ws += w;
        if ((i + 1) % S4B_SPREAD_SLAB == 0 || i + 1 == nT) { zeroSlabs += Ws == 0.0; Ws = 0.0; }
      }
      if (!(W > 0.0)) throw std::invalid_argument(who + ": the weights sum to 0 (no row carries weight)");
      SpreadCall g{};
      ArmsHold hold;
      const int64_t S = contrast_arms(who, ar, peers, in->n_arms == 2, nullptr, g.arms, hold);
      out->weight = W;
      g.arms.rows.info = out->info; g.arms.rows.G = 0; g.arms.rows.weights = nullptr;
      g.nArms = in->n_arms; g.thresholds = in->thresholds; g.T = T; g.binIndex = in->bin_index;
      g.rowWeights = rw->n_weights ? rw->weights : nullptr; g.W = W; g.zeroSlabs = zeroSlabs;
      g.mean = out->mean; g.m2 = out->m2; g.quantiles = ar->n_probs > 0 ? out->quantiles : nullptr; g.draws = out->draws;
      dev_.predict_spread(g);
      out->num_samples = S;
      return S;
    } else throw std::invalid_argument("predict_spread: this device layer has no spread kernels (the across-row read-out is formed by the HIP library only)");
  }
  // s4b_predict_check: posterior predictive checks — per pooled draw the weighted mean, standard deviation, third central moment and extremes of the
  // replicate y_rep ACROSS THE ROWS, the share of the weight above each of up to 64 thresholds and a realised discrepancy beside the observed one; the
  // same statistics of y itself; of the per-draw series the mean, m2 and type-7 quantiles over the draws.  Pooled like predict_ppd.  W and the slabs
  // without weight are formed here, in row order.  Everything is validated here, before any launch.
  int64_t predict_check(const s4b_check_in* in, s4b_check_out* out, const SamplerCore* const* peers) {
    if (!out) throw std::invalid_argument("predict_check: NULL output struct");
    for (int j = 0; j < 8; ++j) out->info[j] = 0;
    out->weight = 0.0;
    const int64_t own = (int64_t)keptScale_.size() / 2;
    out->num_samples = own;
    if (!in || !out->draws) return own;          // query
    {          // (the checks run on every device layer; the layer without check kernels refuses what passed them)
      const std::string who = "predict_check";
      const s4b_summary_in* rw = &in->rows;
      if (rw->n_weights != 0) throw std::invalid_argument(who + ": rows.n_weights must be 0 (the row weights are row_weights), not " + std::to_string(rw->n_weights));
      check_summary_rows(rw, who, 0);
      const int T = in->n_thresholds;
      if (T < 0 || T > S4B_SPREAD_THRESHOLDS_MAX)
        throw std::invalid_argument(who + ": n_thresholds must lie in [0, " + std::to_string(S4B_SPREAD_THRESHOLDS_MAX) + "], not " + std::to_string(T));
      if (T > 0 && rw->link != 0) throw std::invalid_argument(who + ": n_thresholds must be 0 under link 1 (a binary replicate is 0 or 1: its mean is the share of ones), not " + std::to_string(T));
      if (T > 0 && !in->thresholds) throw std::invalid_argument(who + ": NULL thresholds");
      for (int j = 0; j < T; ++j) {
        if (std::isnan(in->thresholds[j])) throw std::invalid_argument(who + ": threshold " + std::to_string(j) + " is a NaN");
        if (j > 0 && !(in->thresholds[j] > in->thresholds[j - 1])) throw std::invalid_argument(who + ": the thresholds are not strictly ascending at index " + std::to_string(j));
      }
      if (in->bin_index < 0 || in->bin_index > 2) throw std::invalid_argument(who + ": bin_index must be 0 (the library's choice), 1 (compares) or 2 (search), not " + std::to_string(in->bin_index));
      if (in->n_probs < 0 || in->n_probs > 16) throw std::invalid_argument(who + ": between 0 and 16 probs per call, not " + std::to_string(in->n_probs));
      if (in->n_probs > 0 && !in->probs) throw std::invalid_argument(who + ": NULL probs");
      for (int j = 0; j < in->n_probs; ++j)
        if (!(in->probs[j] >= 0.0 && in->probs[j] <= 1.0)) throw std::invalid_argument(who + ": prob " + std::to_string(in->probs[j]) + " outside [0, 1]");
      if (in->n_probs > 0 && !out->quantiles) throw std::invalid_argument(who + ": n_probs > 0 needs quantiles");
      if (in->scratch_bytes < 0) throw std::invalid_argument(who + ": negative scratch_bytes");
      if (!in->y) throw std::invalid_argument(who + ": NULL y (a check holds the replicate against the observed responses)");
      const int64_t nT = rw->n_test;
      double W = 0.0, Ws = 0.0;          // in row order, in double: part of the definition
      int64_t zeroSlabs = 0;
      for (int64_t i = 0; i < nT; ++i) {
        const double w = in->row_weights ? in->row_weights[i] : 1.0;
        if (!(w >= 0.0) || std::isinf(w)) throw std::invalid_argument(who + ": weight " + std::to_string(w) + " of row " + std::to_string(i) + " is negative or not finite");
        W += w; Ws += w;
        if ((i + 1) % S4B_SPREAD_SLAB == 0 || i + 1 == nT) { zeroSlabs += Ws == 0.0; Ws = 0.0; }
      }
      if (!(W > 0.0)) throw std::invalid_argument(who + ": the weights sum to 0 (no row carries weight)");
      const int np = in->n_peers;
      const int64_t S = pool_check(who, rw, np, in->peers != nullptr, peers, in->peer_dense_coef, in->peer_ell_coef);
      std::vector<double> sigma;
      check_responses(who, rw, in->y, in->sigma, in->peer_sigma, in->row_scale, np, peers, S, sigma);
      if constexpr (has_predict_check<Dev>::value) {
        std::vector<uint16_t> xb((size_t)P_ * (size_t)nT);
        bin_matrix(rw->x_test, (size_t)nT, xb);
        CheckCall c{};
        c.rows = summary_call(rw, xb, own); c.rows.info = out->info; c.rows.G = 0; c.rows.weights = nullptr;
        c.y = in->y; c.sigma = rw->link == 0 ? sigma.data() : nullptr; c.rowScale = rw->link == 0 ? in->row_scale : nullptr; c.noiseKey = in->noise_key;
        c.thresholds = in->thresholds; c.T = T; c.binIndex = in->bin_index;
        c.rowWeights = in->row_weights; c.W = W; c.zeroSlabs = zeroSlabs;
        c.Q = in->n_probs; c.probs = in->probs; c.scratchBytes = in->scratch_bytes;
        c.mean = out->mean; c.m2 = out->m2; c.quantiles = in->n_probs > 0 ? out->quantiles : nullptr; c.draws = out->draws; c.observed = out->observed;
        DrawPool pool;
        pool_concat(c.rows, pool, rw, xb, np, peers, in->peer_dense_coef, in->peer_ell_coef, S);
        out->weight = W;
        dev_.predict_check(c);
        out->num_samples = S;
        return S;
      } else throw std::invalid_argument("predict_check: this device layer has no check kernels (the replicate is formed by the HIP library only)");
    }
  }
  // s4b_predict_curves: per row the response curve along one or two BART predictors — partial_dependence's v(i,g,k) kept per row instead of averaged
  // over the rows, optionally centred at an anchor grid point — summarised over the pooled draws per (row, grid point), and across the grid per draw
  // (which point is highest / lowest, how far the curve ranges).  Pooled like predict_quantiles.  Everything is validated here, before any launch.
  int64_t predict_curves(const s4b_curves_in* in, s4b_curves_out* out, const SamplerCore* const* peers) {
    if (!out) throw std::invalid_argument("predict_curves: NULL output struct");
    for (int j = 0; j < 8; ++j) out->info[j] = 0;
    const int64_t own = (int64_t)keptScale_.size() / 2;
    out->num_samples = own;
    if (!in) return own;          // query
    {          // (the checks run on every device layer; the layer without curve kernels refuses what passed them)
      const std::string who = "predict_curves";
      const s4b_summary_in* rw = &in->rows;
      if (!out->mean && !out->m2 && !out->quantiles && !out->p_max && !out->p_min && !out->range_mean && !out->range_m2 && !out->range_quantiles)
        throw std::invalid_argument(who + ": nothing asked for (every output is NULL)");
      if (rw->n_weights != 0) throw std::invalid_argument(who + ": rows.n_weights must be 0 (the curves are per row), not " + std::to_string(rw->n_weights));
      check_summary_rows(rw, who, 0);
      if (in->n_vars != 1 && in->n_vars != 2) throw std::invalid_argument(who + ": one or two varied predictors, not " + std::to_string(in->n_vars));
      for (int w = 0; w < in->n_vars; ++w)
        if (in->vars[w] < 0 || in->vars[w] >= P_) throw std::invalid_argument(who + ": predictor " + std::to_string(in->vars[w]) + " outside [0, " + std::to_string(P_) + ")");
      if (in->n_vars == 2 && in->vars[0] == in->vars[1]) throw std::invalid_argument(who + ": the two varied predictors must differ");
      if (in->n_grid < 1 || in->n_grid > 64) throw std::invalid_argument(who + ": between 1 and 64 grid points per call, not " + std::to_string(in->n_grid));
      if (!in->grid) throw std::invalid_argument(who + ": NULL grid");
      const int V = in->n_vars, G = in->n_grid;
      for (int x = 0; x < V * G; ++x) if (std::isnan(in->grid[x])) throw std::invalid_argument(who + ": the grid holds a NaN");
      if (in->anchor < -1 || in->anchor >= G) throw std::invalid_argument(who + ": anchor " + std::to_string(in->anchor) + " outside [-1, " + std::to_string(G) + ")");
      if (in->n_probs < 0 || in->n_probs > 16) throw std::invalid_argument(who + ": between 0 and 16 probs per call, not " + std::to_string(in->n_probs));
      if (in->n_probs > 0 && !in->probs) throw std::invalid_argument(who + ": NULL probs");
      for (int j = 0; j < in->n_probs; ++j)
        if (!(in->probs[j] >= 0.0 && in->probs[j] <= 1.0)) throw std::invalid_argument(who + ": prob " + std::to_string(in->probs[j]) + " outside [0, 1]");
      if (in->n_probs > 0 && !out->quantiles) throw std::invalid_argument(who + ": n_probs > 0 needs quantiles");
      if (in->n_probs == 0 && (out->quantiles || out->range_quantiles)) throw std::invalid_argument(who + ": quantiles or range_quantiles given, but n_probs = 0");
      if (in->scratch_bytes < 0) throw std::invalid_argument(who + ": negative scratch_bytes");
      const int np = in->n_peers;
      const int64_t S = pool_check(who, rw, np, in->peers != nullptr, peers, in->peer_dense_coef, in->peer_ell_coef);
      if ((int64_t)8 * 64 * S * G > S4B_CURVES_SCRATCH_MAX)
        throw std::invalid_argument(who + ": " + std::to_string(S) + " pooled draws x " + std::to_string(G) + " grid points need " + std::to_string((int64_t)8 * 64 * S * G) +
                                    " bytes for the curves of 64 rows, at most " + std::to_string(S4B_CURVES_SCRATCH_MAX) + " (the grid cannot be split: fewer grid points or draws)");
      if constexpr (has_predict_curves<Dev>::value) {
        const int64_t nT = rw->n_test;
        std::vector<uint16_t> xb((size_t)P_ * (size_t)nT);
        bin_matrix(rw->x_test, (size_t)nT, xb);
        std::vector<uint16_t> gridBin((size_t)(V * G));          // bin_matrix's rule: the number of cuts strictly below the value
        for (int w = 0; w < V; ++w) {
          const std::vector<double>& cu = cuts_[(size_t)in->vars[w]];
          for (int g = 0; g < G; ++g) gridBin[(size_t)(w * G + g)] = (uint16_t)(std::lower_bound(cu.begin(), cu.end(), in->grid[w * G + g]) - cu.begin());
        }
        CurvesCall c{};
        c.rows = summary_call(rw, xb, own); c.rows.info = out->info; c.rows.G = 0; c.rows.weights = nullptr;
        c.V = V; c.vars[0] = in->vars[0]; c.vars[1] = V > 1 ? in->vars[1] : -1; c.G = G; c.anchor = in->anchor; c.gridBin = gridBin.data();
        c.Q = in->n_probs; c.probs = in->probs; c.scratchBytes = in->scratch_bytes;
        c.mean = out->mean; c.m2 = out->m2; c.quantiles = in->n_probs > 0 ? out->quantiles : nullptr; c.pMax = out->p_max; c.pMin = out->p_min;
        c.rangeMean = out->range_mean; c.rangeM2 = out->range_m2; c.rangeQuantiles = out->range_quantiles;
        DrawPool pool;
        pool_concat(c.rows, pool, rw, xb, np, peers, in->peer_dense_coef, in->peer_ell_coef, S);
        // the tree order of every pooled draw, each sampler's own trees
        std::vector<int32_t> order, numBase, o, nb;
        for (int x = -1; x < np; ++x) {
          int64_t mx = 0, tot = 0;
          (x < 0 ? this : peers[x])->pd_tree_order(V, in->vars, o, nb, mx, tot);
          order.insert(order.end(), o.begin(), o.end()); numBase.insert(numBase.end(), nb.begin(), nb.end());
          c.maxAffected = std::max(c.maxAffected, mx); c.totalAffected += tot;
        }
        c.order = order.data(); c.numBase = numBase.data();
        dev_.predict_curves(c);
        out->num_samples = S;
        return S;
      } else throw std::invalid_argument("predict_curves: this device layer has no curve kernels (the curves are formed by the HIP library only)");
    }
  }
  // s4b_predict_describe: per row, from its pooled draws in sorted order — one arm: predict_quantiles' value, two arms: predict_contrast's d — the
  // type-7 quantiles and the median, the shortest window of hdi_count[c] draws, the draws strictly above and strictly below each threshold and the
  // median absolute deviation.  Everything is validated here, before any launch; with every output NULL the call is the query for the plan.
  int64_t predict_describe(const s4b_describe_in* in, s4b_describe_out* out, const SamplerCore* const* peers) {
    if (!out) throw std::invalid_argument("predict_describe: NULL output struct");
    for (int j = 0; j < 8; ++j) out->info[j] = 0;
    const int64_t own = (int64_t)keptScale_.size() / 2;
    out->num_samples = own;
    if (!in) return own;          // query: the kept draws of this sampler alone
    {          // (the checks run on every device layer; the layer without the describe kernel refuses what passed them)
      const std::string who = "predict_describe";
      const s4b_contrast_in* ar = &in->arms;
      const s4b_summary_in* rw = &ar->rows;
      if (rw->n_weights != 0) throw std::invalid_argument(who + ": arms.rows.n_weights must be 0 (every output is per row: there are no row weights), not " + std::to_string(rw->n_weights));
      contrast_check_in(who, ar, 0);
      if (in->n_arms != 1 && in->n_arms != 2) throw std::invalid_argument(who + ": n_arms must be 1 (the fitted value) or 2 (the contrast), not " + std::to_string(in->n_arms));
      if (in->n_arms == 1 && (ar->x_test0 || ar->offset0 || ar->dense0 || ar->ell_index0 || ar->ell_value0))
        throw std::invalid_argument(who + ": n_arms = 1 takes no arm-0 pointer (x_test0, offset0, dense0, ell_index0, ell_value0 must be NULL)");
      const int M = in->n_hdi, T = in->n_thresholds;
      if (M < 0 || M > S4B_DESCRIBE_HDI_MAX) throw std::invalid_argument(who + ": n_hdi must lie in [0, " + std::to_string(S4B_DESCRIBE_HDI_MAX) + "], not " + std::to_string(M));
      if (M > 0 && !in->hdi_count) throw std::invalid_argument(who + ": NULL hdi_count");
      if (T < 0 || T > S4B_DESCRIBE_THRESHOLDS_MAX)
        throw std::invalid_argument(who + ": n_thresholds must lie in [0, " + std::to_string(S4B_DESCRIBE_THRESHOLDS_MAX) + "], not " + std::to_string(T));
      if (T > 0 && !in->thresholds) throw std::invalid_argument(who + ": NULL thresholds");
      for (int j = 0; j < T; ++j) if (std::isnan(in->thresholds[j])) throw std::invalid_argument(who + ": threshold " + std::to_string(j) + " is a NaN");
      if (out->quantiles && ar->n_probs == 0) throw std::invalid_argument(who + ": quantiles given, but n_probs = 0");
      if ((out->hdi || out->hdi_start) && M == 0) throw std::invalid_argument(who + ": hdi or hdi_start given, but n_hdi = 0");
      if ((out->n_above || out->n_below) && T == 0) throw std::invalid_argument(who + ": n_above or n_below given, but n_thresholds = 0");
      DescribeCall g{};
      ArmsHold hold;
      const int64_t S = contrast_arms(who, ar, peers, in->n_arms == 2, out->info, g.arms, hold);
      for (int j = 0; j < M; ++j)
        if (in->hdi_count[j] < 1 || in->hdi_count[j] > S)
          throw std::invalid_argument(who + ": hdi_count " + std::to_string(in->hdi_count[j]) + " outside [1, " + std::to_string(S) + "] (the pooled draws)");
      if constexpr (has_predict_describe<Dev>::value) {
        g.arms.rows.G = 0; g.arms.rows.weights = nullptr;
        g.nArms = in->n_arms; g.nMass = M; g.hdiCount = in->hdi_count; g.nThr = T; g.thresholds = in->thresholds;
        g.quantiles = out->quantiles; g.median = out->median; g.hdi = out->hdi; g.hdiStart = out->hdi_start;
        g.nAbove = out->n_above; g.nBelow = out->n_below; g.mad = out->mad;
        dev_.predict_describe(g);
        out->num_samples = S;
        return S;
      } else throw std::invalid_argument("predict_describe: this device layer has no describe kernel (the per-row description is formed by the HIP library only)");
    }
  }
  // s4b_predict_sorted: per pooled draw the order statistics of the rows' values ACROSS THE ROWS — one arm: predict_quantiles' value, two arms:
  // predict_contrast's d — as type-7 quantiles at the row probs and as the order statistics at the cut ranks themselves; of those series the mean, m2
  // and type-7 quantiles over the draws; per row and cut the draws in which the row lies strictly above and strictly below the cut.  Everything is
  // validated here, before any launch; with every output NULL the call is the query for the plan.
  int64_t predict_sorted(const s4b_sorted_in* in, s4b_sorted_out* out, const SamplerCore* const* peers) {
    if (!out) throw std::invalid_argument("predict_sorted: NULL output struct");
    for (int j = 0; j < 8; ++j) out->info[j] = 0;
    const int64_t own = (int64_t)keptScale_.size() / 2;
    out->num_samples = own;
    if (!in) return own;          // query: the kept draws of this sampler alone
    {          // (the checks run on every device layer; the layer without the kernels refuses what passed them)
      const std::string who = "predict_sorted";
      const s4b_contrast_in* ar = &in->arms;
      const s4b_summary_in* rw = &ar->rows;
      if (rw->n_weights != 0) throw std::invalid_argument(who + ": arms.rows.n_weights must be 0 (ranks across the rows are unweighted: there are no row weights), not " + std::to_string(rw->n_weights));
      contrast_check_in(who, ar, 0);
      if (rw->n_test >= ((int64_t)1 << 31)) throw std::invalid_argument(who + ": n_test must be below 2^31 (a rank is a 32-bit integer), not " + std::to_string(rw->n_test));
      if (in->n_arms != 1 && in->n_arms != 2) throw std::invalid_argument(who + ": n_arms must be 1 (the fitted value) or 2 (the contrast), not " + std::to_string(in->n_arms));
      if (in->n_arms == 1 && (ar->x_test0 || ar->offset0 || ar->dense0 || ar->ell_index0 || ar->ell_value0))
        throw std::invalid_argument(who + ": n_arms = 1 takes no arm-0 pointer (x_test0, offset0, dense0, ell_index0, ell_value0 must be NULL)");
      const int Qr = in->n_row_probs, J = in->n_cuts;
      if (Qr < 0 || Qr > S4B_SORTED_PROBS_MAX)
        throw std::invalid_argument(who + ": n_row_probs must lie in [0, " + std::to_string(S4B_SORTED_PROBS_MAX) + "], not " + std::to_string(Qr));
      if (Qr > 0 && !in->row_probs) throw std::invalid_argument(who + ": NULL row_probs");
      for (int j = 0; j < Qr; ++j)
        if (!(in->row_probs[j] >= 0.0 && in->row_probs[j] <= 1.0)) throw std::invalid_argument(who + ": row prob " + std::to_string(in->row_probs[j]) + " outside [0, 1]");
      if (J < 0 || J > S4B_SORTED_CUTS_MAX) throw std::invalid_argument(who + ": n_cuts must lie in [0, " + std::to_string(S4B_SORTED_CUTS_MAX) + "], not " + std::to_string(J));
      if (J > 0 && !in->cut_rank) throw std::invalid_argument(who + ": NULL cut_rank");
      for (int j = 0; j < J; ++j)
        if (in->cut_rank[j] < 0 || in->cut_rank[j] >= rw->n_test)
          throw std::invalid_argument(who + ": cut_rank " + std::to_string(in->cut_rank[j]) + " outside [0, " + std::to_string(rw->n_test - 1) + "] (the rows)");
      if ((out->mean || out->m2 || out->draws || out->quantiles) && Qr + J == 0) throw std::invalid_argument(who + ": mean, m2, quantiles or draws given, but n_row_probs + n_cuts = 0");
      if (out->quantiles && ar->n_probs == 0) throw std::invalid_argument(who + ": quantiles given, but n_probs = 0");
      if ((out->n_above || out->n_below) && J == 0) throw std::invalid_argument(who + ": n_above or n_below given, but n_cuts = 0");
      SortedCall g{};
      ArmsHold hold;
      const int64_t S = contrast_arms(who, ar, peers, in->n_arms == 2, out->info, g.arms, hold);
      if constexpr (has_predict_sorted<Dev>::value) {
        g.arms.rows.G = 0; g.arms.rows.weights = nullptr;
        g.nArms = in->n_arms; g.Qr = Qr; g.rowProbs = in->row_probs; g.J = J; g.cutRank = in->cut_rank;
        g.mean = out->mean; g.m2 = out->m2; g.quantiles = out->quantiles; g.draws = out->draws; g.nAbove = out->n_above; g.nBelow = out->n_below;
        dev_.predict_sorted(g);
        out->num_samples = S;
        return S;
      } else throw std::invalid_argument("predict_sorted: this device layer has no selection kernels (the order statistics across the rows are formed by the HIP library only)");
    }
  }
  // TEST ENTRY (s4b_test_sorted_select): the selection and the count kernels of predict_sorted alone on the caller's matrix; the checks run on every layer
  void test_sorted_select(const double* values, int64_t n, int64_t S, int64_t blockDraws, int nRanks, const int32_t* ranks, double* orderStats, int nCuts,
                          const int32_t* cutRank, int32_t* nAbove, int32_t* nBelow, int64_t* info) {
    const std::string who = "test_sorted_select";
    if (!values || !info) throw std::invalid_argument(who + ": NULL values or info");
    for (int j = 0; j < 8; ++j) info[j] = 0;
    if (n < 1 || n >= ((int64_t)1 << 31)) throw std::invalid_argument(who + ": n must lie in [1, 2^31), not " + std::to_string(n));
    if (S < 1 || S > 16384) throw std::invalid_argument(who + ": S must lie in [1, 16384], not " + std::to_string(S));
    if (blockDraws < 1 || std::min(blockDraws, S) > 1024) throw std::invalid_argument(who + ": block_draws must be at least 1 and a block at most 1024 draws, not " + std::to_string(blockDraws));
    if (nRanks < 0 || nRanks > 32) throw std::invalid_argument(who + ": n_ranks must lie in [0, 32], not " + std::to_string(nRanks));
    if (nCuts < 0 || nCuts > S4B_SORTED_CUTS_MAX) throw std::invalid_argument(who + ": n_cuts must lie in [0, " + std::to_string(S4B_SORTED_CUTS_MAX) + "], not " + std::to_string(nCuts));
    if (nRanks + nCuts == 0) throw std::invalid_argument(who + ": neither ranks nor cuts");
    if ((nRanks > 0 && !ranks) || (nCuts > 0 && !cutRank)) throw std::invalid_argument(who + ": NULL ranks or cut_rank");
    std::vector<int32_t> all;
    for (int j = 0; j < nRanks + nCuts; ++j) {
      const int32_t r = j < nRanks ? ranks[j] : cutRank[j - nRanks];
      if (r < 0 || r >= n) throw std::invalid_argument(who + ": rank " + std::to_string(r) + " outside [0, " + std::to_string(n - 1) + "]");
      all.push_back(r);
    }
    std::sort(all.begin(), all.end());
    if (std::unique(all.begin(), all.end()) - all.begin() > 32) throw std::invalid_argument(who + ": more than 32 distinct ranks among ranks and cut_rank");
    for (size_t x = 0, m = (size_t)n * (size_t)S; x < m; ++x) if (!std::isfinite(values[x])) throw std::invalid_argument(who + ": values holds a value that is not finite");
    if constexpr (has_test_sorted_select<Dev>::value) {
      SortedSelectCall c{values, n, S, blockDraws, nRanks, ranks, orderStats, nCuts, cutRank, nAbove, nBelow, info};
      dev_.test_sorted_select(c);
    } else throw std::invalid_argument("test_sorted_select: this device layer has no selection kernels");
  }
  // s4b_predict_ppd: the posterior predictive distribution of new observations at the rows — type-7 quantiles of y_rep = z + sigma row_scale e — and the
  // scores of held-out responses y (log predictive density, mean and squared deviations of the pointwise log-likelihood, PIT), per row over the
  // pooled draws.  Pooled like predict_quantiles.  Everything is validated here, before any launch.
  int64_t predict_ppd(const s4b_ppd_in* in, s4b_ppd_out* out, const SamplerCore* const* peers) {
    if (!out) throw std::invalid_argument("predict_ppd: NULL output struct");
    for (int j = 0; j < 8; ++j) out->info[j] = 0;
    const int64_t own = (int64_t)keptScale_.size() / 2;
    out->num_samples = own;
    if (!in || (!out->quantiles && !out->lpd && !out->lmean && !out->lm2 && !out->pit)) return own;          // query
    if constexpr (has_predict_ppd<Dev>::value) {
      const std::string who = "predict_ppd";
      const s4b_summary_in* rw = &in->rows;
      if (rw->n_weights != 0) throw std::invalid_argument(who + ": n_weights must be 0 (every output is per row), not " + std::to_string(rw->n_weights));
      check_summary_rows(rw, who, 0);
      if (in->n_probs < 0 || in->n_probs > 16) throw std::invalid_argument(who + ": between 0 and 16 probs per call, not " + std::to_string(in->n_probs));
      if (in->n_probs > 0 && rw->link != 0)
        throw std::invalid_argument(who + ": n_probs > 0 under link 1: no y_rep is formed for a binary response, a row's predictive distribution is Bernoulli(mean of ev), which predict_summary gives");
      if (in->n_probs > 0 && !in->probs) throw std::invalid_argument(who + ": NULL probs");
      for (int j = 0; j < in->n_probs; ++j)
        if (!(in->probs[j] >= 0.0 && in->probs[j] <= 1.0)) throw std::invalid_argument(who + ": prob " + std::to_string(in->probs[j]) + " outside [0, 1]");
      if (in->n_probs > 0 && !out->quantiles) throw std::invalid_argument(who + ": n_probs > 0 needs quantiles");
      if (in->scratch_bytes < 0) throw std::invalid_argument(who + ": negative scratch_bytes");
      if ((out->lmean == nullptr) != (out->lm2 == nullptr)) throw std::invalid_argument(who + ": lmean and lm2 are given together or not at all");
      const bool scores = out->lpd || out->lmean || out->pit;
      if (scores && !in->y) throw std::invalid_argument(who + ": lpd, lmean, lm2 and pit need y");
      if (out->pit && rw->link != 0) throw std::invalid_argument(who + ": pit must be NULL under link 1 (the PIT of a binary response is not formed)");
      if (in->n_probs == 0 && !(in->y && scores)) throw std::invalid_argument(who + ": nothing asked for (no probs, no y with a score output)");
      const int64_t nT = rw->n_test;
      const int np = in->n_peers;
      const int64_t S = pool_check(who, rw, np, in->peers != nullptr, peers, in->peer_dense_coef, in->peer_ell_coef);
      // sigma per pooled draw, the row scale, the responses
      std::vector<double> sigma;
      check_responses(who, rw, in->y, in->sigma, in->peer_sigma, in->row_scale, np, peers, S, sigma);
      std::vector<uint16_t> xb((size_t)P_ * (size_t)nT);
      bin_matrix(rw->x_test, (size_t)nT, xb);
      PpdCall c{};
      c.rows = summary_call(rw, xb, own); c.rows.info = out->info; c.rows.G = 0; c.rows.weights = nullptr;
      c.y = in->y; c.sigma = rw->link == 0 ? sigma.data() : nullptr; c.rowScale = rw->link == 0 ? in->row_scale : nullptr; c.noiseKey = in->noise_key;
      c.Q = in->n_probs; c.probs = in->probs; c.scratchBytes = in->scratch_bytes; c.quantiles = in->n_probs > 0 ? out->quantiles : nullptr;
      c.lpd = out->lpd; c.lmean = out->lmean; c.lm2 = out->lm2; c.pit = out->pit;
      DrawPool pool;
      pool_concat(c.rows, pool, rw, xb, np, peers, in->peer_dense_coef, in->peer_ell_coef, S);
      dev_.predict_ppd(c);
      out->num_samples = S;
      return S;
    } else throw std::invalid_argument("predict_ppd: this device layer has no posterior predictive kernels (the read-out is formed by the HIP library only)");
  }
  // the default tail length of PSIS over S pooled draws: min(ceil(S / 5), ceil(3 sqrt S)) — loo's ceiling(min(0.2 S, 3 sqrt(S / r_eff))) at r_eff = 1 —
  // with ceil(3 sqrt S) the smallest m with m m >= 9 S, formed in integers
  static int64_t loo_tail_len(int64_t S) {
    int64_t m = (int64_t)std::floor(3.0 * std::sqrt((double)S));
    while (m > 0 && (m - 1) * (m - 1) >= 9 * S) --m;
    while (m * m < 9 * S) ++m;
    return std::min((S + 4) / 5, m);
  }
  // s4b_predict_loo: PSIS-LOO of held-out (or the training) responses y per row over the pooled draws — elpd_loo, the Pareto shape khat of the
  // importance ratios' tail, the lpd and the effective sample size of the smoothed weights.  Pooled and validated like predict_ppd, before any launch.
  int64_t predict_loo(const s4b_loo_in* in, s4b_loo_out* out, const SamplerCore* const* peers) {
    if (!out) throw std::invalid_argument("predict_loo: NULL output struct");
    for (int j = 0; j < 8; ++j) out->info[j] = 0;
    const int64_t own = (int64_t)keptScale_.size() / 2;
    out->num_samples = own; out->tail_len = 0;
    if (!in || (!out->elpd_loo && !out->pareto_k && !out->lpd && !out->ess)) return own;          // query
    if constexpr (has_predict_loo<Dev>::value) {
      const std::string who = "predict_loo";
      const s4b_summary_in* rw = &in->rows;
      if (rw->n_weights != 0) throw std::invalid_argument(who + ": n_weights must be 0 (every output is per row), not " + std::to_string(rw->n_weights));
      check_summary_rows(rw, who, 0);
      if (in->scratch_bytes < 0) throw std::invalid_argument(who + ": negative scratch_bytes");
      if (!in->y) throw std::invalid_argument(who + ": NULL y (the importance ratios are those of the responses)");
      const int64_t nT = rw->n_test;
      const int np = in->n_peers;
      const int64_t S = pool_check(who, rw, np, in->peers != nullptr, peers, in->peer_dense_coef, in->peer_ell_coef);
      const int64_t most = std::min<int64_t>(S - 1, 1024);
      if (in->tail_len != 0 && (in->tail_len < 5 || in->tail_len > most))
        throw std::invalid_argument(who + ": tail_len " + std::to_string(in->tail_len) + " outside [5, " + std::to_string(most) + "] (0: the default; at most 1024 and the pooled draws - 1, " + std::to_string(S) + " here)");
      std::vector<double> sigma;
      check_responses(who, rw, in->y, in->sigma, in->peer_sigma, in->row_scale, np, peers, S, sigma);
      std::vector<uint16_t> xb((size_t)P_ * (size_t)nT);
      bin_matrix(rw->x_test, (size_t)nT, xb);
      LooCall c{};
      c.rows = summary_call(rw, xb, own); c.rows.info = out->info; c.rows.G = 0; c.rows.weights = nullptr;
      c.y = in->y; c.sigma = rw->link == 0 ? sigma.data() : nullptr; c.rowScale = rw->link == 0 ? in->row_scale : nullptr;
      c.tailLen = (int)(in->tail_len != 0 ? in->tail_len : loo_tail_len(S)); c.scratchBytes = in->scratch_bytes;
      c.elpd = out->elpd_loo; c.khat = out->pareto_k; c.lpd = out->lpd; c.ess = out->ess;
      DrawPool pool;
      pool_concat(c.rows, pool, rw, xb, np, peers, in->peer_dense_coef, in->peer_ell_coef, S);
      dev_.predict_loo(c);
      out->num_samples = S; out->tail_len = c.tailLen;
      return S;
    } else throw std::invalid_argument("predict_loo: this device layer has no PSIS-LOO kernels (the read-out is formed by the HIP library only)");
  }
  // the chains of s4b_predict_convergence: `lens` the kept draws of the pooled samplers in pooled order.  Every chain keeps its first N0 = min lens
  // draws; split: its first and its last floor(N0 / 2) of those.  Returns the common length N, the first draws inside the pooled row in `start`.
  static int conv_chains(const std::vector<int64_t>& lens, bool split, std::vector<int32_t>& start) {
    const int64_t n0 = *std::min_element(lens.begin(), lens.end()), h = n0 / 2;
    int64_t at = 0;
    start.clear();
    for (int64_t n : lens) {
      start.push_back((int32_t)at);
      if (split) start.push_back((int32_t)(at + n0 - h));
      at += n;
    }
    return (int)(split ? h : n0);
  }
  // s4b_predict_convergence: split R-hat, the effective sample size, the pooled mean and its Monte-Carlo standard error per row with the chains kept
  // apart — every pooled sampler one chain.  Pooled and validated like predict_loo, before any launch.
  int64_t predict_convergence(const s4b_conv_in* in, s4b_conv_out* out, const SamplerCore* const* peers) {
    if (!out) throw std::invalid_argument("predict_convergence: NULL output struct");
    for (int j = 0; j < 8; ++j) out->info[j] = 0;
    const int64_t own = (int64_t)keptScale_.size() / 2;
    out->num_samples = own; out->n_chains = 0; out->chain_len = 0;
    if (!in || (!out->rhat && !out->ess && !out->mean && !out->mcse && !out->n_pairs)) return own;          // query
    if constexpr (has_predict_convergence<Dev>::value) {
      const std::string who = "predict_convergence";
      const s4b_summary_in* rw = &in->rows;
      if (rw->n_weights != 0) throw std::invalid_argument(who + ": n_weights must be 0 (every output is per row), not " + std::to_string(rw->n_weights));
      check_summary_rows(rw, who, 0);
      if (in->scratch_bytes < 0) throw std::invalid_argument(who + ": negative scratch_bytes");
      if (in->quantity != 0 && in->quantity != 1) throw std::invalid_argument(who + ": quantity must be 0 (the fitted value) or 1 (the likelihood of y), not " + std::to_string(in->quantity));
      if (in->split != 0 && in->split != 1) throw std::invalid_argument(who + ": split must be 0 or 1, not " + std::to_string(in->split));
      if (in->quantity == 1 && !in->y) throw std::invalid_argument(who + ": NULL y (quantity 1 is the likelihood of the responses)");
      if (in->quantity == 0 && in->y) throw std::invalid_argument(who + ": quantity 0 takes no y");
      const int64_t nT = rw->n_test;
      const int np = in->n_peers;
      const int64_t S = pool_check(who, rw, np, in->peers != nullptr, peers, in->peer_dense_coef, in->peer_ell_coef);
      const int64_t numChains = (int64_t)(np + 1) * (in->split ? 2 : 1);
      if (numChains > 256) throw std::invalid_argument(who + ": " + std::to_string(numChains) + " chains, at most 256 (" + std::to_string(np + 1) + " pooled samplers" + (in->split ? ", each split in two)" : ")"));
      std::vector<double> sigma;
      if (in->quantity == 1) check_responses(who, rw, in->y, in->sigma, in->peer_sigma, in->row_scale, np, peers, S, sigma);
      std::vector<int64_t> lens{own};
      for (int x = 0; x < np; ++x) lens.push_back((int64_t)peers[x]->keptScale_.size() / 2);
      std::vector<int32_t> start;
      const int N = conv_chains(lens, in->split != 0, start);
      std::vector<uint16_t> xb((size_t)P_ * (size_t)nT);
      bin_matrix(rw->x_test, (size_t)nT, xb);
      ConvCall c{};
      c.rows = summary_call(rw, xb, own); c.rows.info = out->info; c.rows.G = 0; c.rows.weights = nullptr;
      c.quantity = in->quantity;
      if (in->quantity == 1) { c.y = in->y; c.sigma = rw->link == 0 ? sigma.data() : nullptr; c.rowScale = rw->link == 0 ? in->row_scale : nullptr; }
      c.numChains = (int)numChains; c.chainLen = N; c.chainStart = start.data(); c.scratchBytes = in->scratch_bytes;
      c.rhat = out->rhat; c.ess = out->ess; c.mean = out->mean; c.mcse = out->mcse; c.nPairs = out->n_pairs;
      DrawPool pool;
      pool_concat(c.rows, pool, rw, xb, np, peers, in->peer_dense_coef, in->peer_ell_coef, S);
      if (N < 1) {          // a chain of one draw, split: nothing to launch, every row without an answer
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (double* o : {out->rhat, out->ess, out->mean, out->mcse}) if (o) std::fill(o, o + nT, nan);
        if (out->n_pairs) std::fill(out->n_pairs, out->n_pairs + nT, -1);
      } else dev_.predict_convergence(c);
      out->num_samples = S; out->n_chains = (int32_t)numChains; out->chain_len = N;
      return S;
    } else throw std::invalid_argument("predict_convergence: this device layer has no chain kernels (the read-out is formed by the HIP library only)");
  }
  // ---- sampler state as a byte string (layout: include/stan4bart_amd.h, s4b_get_state)
  int64_t get_state(void* buf, int64_t cap) {
    live();
    const int D = model_->sp.D;
    HostTrees h; download_trees(h);
    std::vector<std::vector<int32_t>> nodes((size_t)T_); std::vector<std::vector<double>> leafMu((size_t)T_);
    size_t treeBytes = 0;
    for (int t = 0; t < T_; ++t) {
      TreeView tv = h.view(t, nc_);
      int nd, k; Walker<TreeView> w(tv, 0);
      while (w.next(nd, k)) {
        if (k == 2) continue;
        if (k == 1) { nodes[(size_t)t].push_back(tv.var.get(nd)); nodes[(size_t)t].push_back((int32_t)tv.cut.get(nd)); }
        else { nodes[(size_t)t].push_back(-1); nodes[(size_t)t].push_back(h.cnt[(size_t)t * nc_ + nd]); leafMu[(size_t)t].push_back(h.mu[(size_t)t * nc_ + nd]); }
      }
      treeBytes += 8 + nodes[(size_t)t].size() * 4 + leafMu[(size_t)t].size() * 8;
    }
    const size_t need = sizeof(s4b_state_header) + (size_t)(4 * D + 6 + 7) * 8 + (8 + 2 + 626) * 4 + 4 * 8 + (size_t)(binary_ ? 3 : 2) * n_ * 8 + treeBytes + (latMode_ ? 16 : 0);
    if (!buf || cap < (int64_t)need) return (int64_t)need;
    unsigned char* o = (unsigned char*)buf;
    auto put = [&](const void* src, size_t k) { if (k) std::memcpy(o, src, k); o += k; };
    s4b_state_header hd; std::memset(&hd, 0, sizeof(hd));
    hd.magic = S4B_STATE_MAGIC; hd.version = 1; hd.n = (int64_t)n_; hd.n_trees = T_; hd.num_unconstrained = D; hd.is_binary = binary_ ? 1 : 0; hd.p = P_;
    if (kModeled_) { const double kk = dev_.k_current(); std::memcpy(&hd.reserved[0], &kk, 8); }
    hd.reserved[1] = latMode_;
    put(&hd, sizeof(hd));
    Nuts::State ns; nuts_->get_state(ns);
    put(ns.q.data(), (size_t)D * 8); put(ns.inv_metric.data(), (size_t)D * 8); put(ns.wm.data(), (size_t)D * 8); put(ns.wm2.data(), (size_t)D * 8);
    const double sc6[6] = {ns.stepsize, ns.mu, ns.counter, ns.s_bar, ns.x_bar, ns.wn};
    put(sc6, sizeof(sc6)); put(ns.last, sizeof(ns.last));
    uint32_t win[8]; for (int i = 0; i < 7; ++i) win[i] = ns.window[i]; win[7] = (uint32_t)ns.adapting;
    put(win, sizeof(win)); put(ns.rng, sizeof(ns.rng));
    uint32_t rr[626]; get_rng(rr); rr[625] = 0u;
    put(rr, sizeof(rr));
    ScaleState scl; dev_.get_scale(scl);
    const double sc4[4] = {scl.min, scl.max, scl.range, scl.sigmaData};
    put(sc4, sizeof(sc4));
    std::vector<double> off(n_), R(n_), aux(n_);
    dev_.download_obs(OBS_OFF, off.data()); dev_.download_obs(OBS_R, R.data());
    dev_.download_obs(binary_ ? OBS_LAT : OBS_Y, aux.data());
    put(off.data(), n_ * 8);
    if (binary_) { for (size_t i = 0; i < n_; ++i) R[i] = aux[i] - R[i]; }
    else for (size_t i = 0; i < n_; ++i) R[i] = ((aux[i] - off[i] - scl.min) / scl.range - 0.5) - R[i];
    put(R.data(), n_ * 8);
    if (binary_) put(aux.data(), n_ * 8);
    for (int t = 0; t < T_; ++t) {
      const int32_t cnt[2] = {(int32_t)(nodes[(size_t)t].size() / 2), (int32_t)leafMu[(size_t)t].size()};
      put(cnt, sizeof(cnt)); put(nodes[(size_t)t].data(), nodes[(size_t)t].size() * 4); put(leafMu[(size_t)t].data(), leafMu[(size_t)t].size() * 8);
    }
    if (latMode_) { uint64_t ls[2]; dev_latent_state(ls); put(ls, sizeof(ls)); }
    return (int64_t)need;
  }
  void set_state(const void* buf, int64_t size) {
    live();
    const int D = model_->sp.D;
    Reader r{(const unsigned char*)buf, (size_t)(size < 0 ? 0 : size), 0};
    r.what = "sampler state: truncated";
    s4b_state_header hd;
    if (!buf) throw std::invalid_argument("set_state: NULL buffer");
    r.get(&hd, sizeof(hd));
    if (hd.magic != S4B_STATE_MAGIC) throw std::invalid_argument("not a stan4bart sampler state");
    if (hd.version != 1u) throw std::invalid_argument("sampler state: unknown version");
    if (hd.n != (int64_t)n_ || hd.n_trees != T_ || hd.num_unconstrained != D || (hd.is_binary != 0) != binary_ || hd.p != P_)
      throw std::invalid_argument("sampler state: dimensions do not match this sampler");
    if (hd.reserved[1] != (int64_t)latMode_)       // (symmetric, like the k flag below: neither mode's chain is continued by the other's draw)
      throw std::invalid_argument("sampler state: it was written in latent mode " + std::to_string(hd.reserved[1]) + ", this sampler is in latent mode " +
                                  std::to_string(latMode_) + " (set_latent_mode before set_state)");
    Nuts::State ns;
    ns.q.resize((size_t)D); ns.inv_metric.resize((size_t)D); ns.wm.resize((size_t)D); ns.wm2.resize((size_t)D);
    r.get(ns.q.data(), (size_t)D * 8); r.get(ns.inv_metric.data(), (size_t)D * 8); r.get(ns.wm.data(), (size_t)D * 8); r.get(ns.wm2.data(), (size_t)D * 8);
    double sc6[6]; r.get(sc6, sizeof(sc6)); r.get(ns.last, sizeof(ns.last));
    ns.stepsize = sc6[0]; ns.mu = sc6[1]; ns.counter = sc6[2]; ns.s_bar = sc6[3]; ns.x_bar = sc6[4]; ns.wn = sc6[5];
    uint32_t win[8]; r.get(win, sizeof(win)); r.get(ns.rng, sizeof(ns.rng));
    for (int i = 0; i < 7; ++i) ns.window[i] = win[i];
    ns.adapting = (int32_t)win[7];
    uint32_t rr[626]; r.get(rr, sizeof(rr));
    if (rr[0] > 624u) throw std::invalid_argument("sampler state: generator position out of range");
    double sc4[4]; r.get(sc4, sizeof(sc4));
    if (!(sc4[2] > 0.0) || !(sc4[3] > 0.0)) throw std::invalid_argument("sampler state: response range and sigma must be positive");
    std::vector<double> off(n_), fits(n_), lat;
    r.get(off.data(), n_ * 8); r.get(fits.data(), n_ * 8);
    if (binary_) { lat.resize(n_); r.get(lat.data(), n_ * 8); }
    // trees: preorder -> node slots in preorder (slot ids carry no meaning: every move addresses nodes by traversal order)
    HostTrees h; h.alloc(T_, nc_);
    for (int t = 0; t < T_; ++t) {
      int32_t cnt[2]; r.get(cnt, sizeof(cnt));
      if (cnt[0] < 1 || cnt[0] > nc_ || cnt[1] < 1 || 2 * cnt[1] - 1 != cnt[0]) throw std::invalid_argument("sampler state: tree does not fit node_capacity");
      std::vector<int32_t> nd((size_t)cnt[0] * 2); std::vector<double> mu((size_t)cnt[1]);
      r.get(nd.data(), nd.size() * 4); r.get(mu.data(), mu.size() * 8);
      const size_t o = (size_t)t * nc_;
      int leaf = 0; std::vector<int> open;   // parents still waiting for their right child
      for (int i = 0; i < cnt[0]; ++i) {
        int par = -1;
        if (i > 0) {
          if (open.empty()) throw std::invalid_argument("sampler state: malformed tree");
          par = open.back();
          if (h.left[o + (size_t)par] < 0) h.left[o + (size_t)par] = (int16_t)i; else { h.right[o + (size_t)par] = (int16_t)i; open.pop_back(); }
        }
        h.parent[o + (size_t)i] = (int16_t)par;
        const int32_t v = nd[(size_t)2 * i], s2 = nd[(size_t)2 * i + 1];
        if (v >= 0) {
          if (v >= P_ || s2 < 0 || s2 >= numCuts_[(size_t)v]) throw std::invalid_argument("sampler state: rule out of range");
          h.var[o + (size_t)i] = (int16_t)v; h.cut[o + (size_t)i] = (uint16_t)s2; open.push_back(i);
        } else {
          if (leaf >= cnt[1]) throw std::invalid_argument("sampler state: malformed tree");
          h.var[o + (size_t)i] = NODE_LEAF; h.mu[o + (size_t)i] = mu[(size_t)leaf++]; h.cnt[o + (size_t)i] = s2;
        }
      }
      if (!open.empty() || leaf != cnt[1]) throw std::invalid_argument("sampler state: malformed tree");
      h.hwm[(size_t)t] = cnt[0];
    }
    uint64_t ls[2] = {0, 0};
    if (latMode_) { ls[0] = r.u64(); ls[1] = r.u64(); }
    // nothing non-finite reaches the device or the adaptation state (the blob may come from a file or another process)
    {
      auto finite = [](const double* x, size_t k) { for (size_t i = 0; i < k; ++i) if (!std::isfinite(x[i])) return false; return true; };
      bool ok = finite(ns.q.data(), (size_t)D) && finite(ns.inv_metric.data(), (size_t)D) && finite(ns.wm.data(), (size_t)D) && finite(ns.wm2.data(), (size_t)D) &&
                finite(sc6, 6) && finite(sc4, 4) && finite(off.data(), n_) && finite(fits.data(), n_) && (!binary_ || finite(lat.data(), n_)) &&
                finite(h.mu.data(), h.mu.size());
      for (int i = 0; i < 7 && ok; ++i) ok = !std::isnan(ns.last[i]);           // (energy__ / lp__ may legitimately be infinite)
      for (int i = 0; i < D && ok; ++i) ok = ns.inv_metric[(size_t)i] > 0.0;
      if (!ok || !(sc6[0] > 0.0)) throw std::invalid_argument("sampler state: non-finite value, non-positive step size or inverse metric");
    }
    double kState = 0.0;
    std::memcpy(&kState, &hd.reserved[0], 8);
    if (kModeled_) {
      if (!(kState > 0.0) || !std::isfinite(kState)) throw std::invalid_argument("sampler state: k must be positive and finite (the state of a sampler with a fixed k carries none)");
    } else if (kState != 0.0) throw std::invalid_argument("sampler state: it carries the value of a modeled k, this sampler's k is fixed");
    // ---- commit
    if (kModeled_) dev_.set_k(kState);
    if (latMode_) dev_set_latent_state(ls);
    nuts_->set_state(ns);
    dev_.reset_fused_scales();
    nuts_->current_row(row_.data());
    set_rng(rr);
    sigma_ = sc4[3];
    dev_.set_scale(sc4[0], sc4[1], sc4[2], sc4[3]);
    dev_.upload_obs(OBS_OFF, off.data());
    if (binary_) { dev_.upload_obs(OBS_LAT, lat.data()); for (size_t i = 0; i < n_; ++i) fits[i] = lat[i] - fits[i]; }
    else {
      std::vector<double> y(n_); dev_.download_obs(OBS_Y, y.data());
      for (size_t i = 0; i < n_; ++i) fits[i] = ((y[i] - off[i] - sc4[0]) / sc4[2] - 0.5) - fits[i];
    }
    dev_.upload_obs(OBS_R, fits.data());
    dev_.upload_trees(h.var.data(), h.cut.data(), h.left.data(), h.right.data(), h.parent.data(), h.mu.data(), h.hwm.data());
    dev_.upload_counts(h.cnt.data());
    dev_.assign_leaves_only();
    dev_.stan_inputs(stan_mode(), false, cX_.data(), cZ_.data(), &s0_, nullptr);
    check_device();
  }

  void set_trace(bool on) { live(); dev_.set_trace(on); }
  void set_device_sharing(int chains) { live(); dev_.set_device_sharing(chains); }
  int hmc_mode() const { live(); return hmcMode_; }
  void set_hmc_mode(int mode) {
    live();
    if (mode != 0 && mode != 1) throw std::invalid_argument("hmc_mode must be 0 (sufficient statistics) or 1 (one device evaluation per leapfrog)");
    if (mode == 0 && !haveGram_) throw std::invalid_argument("this sampler was created with hmc_mode 1: it has no Gram matrix to evaluate from sufficient statistics");
    hmcMode_ = mode;
    sync_runahead();
  }
  // run-ahead helpers (s4b_set_nuts_helpers / s4b_get_nuts_runahead)
  void set_nuts_helpers(int n) {
    live();
    if (n < 0 || (n & ~16) > 2) throw std::invalid_argument("nuts helpers must be 0 (none), 1 (the backward direction) or 2 (both directions), plus 16 to wait for a helper");
    if (nuts_) nuts_->set_helpers(n & 3, (n & 16) != 0);
  }
  void nuts_runahead(int64_t out[4]) { live(); for (int i = 0; i < 4; ++i) out[i] = 0; if (nuts_) nuts_->runahead_counters(out); }
  // latent mode (s4b_set_latent_mode): 0 = the reference's draw from R's stream, 1 = parallel draw under the chain's Philox key
  static constexpr bool kLatentMode = has_latent_mode<Dev>::value;
  int latent_mode() const { live(); return latMode_; }
  void set_latent_mode(int mode) {
    live();
    if (mode != 0 && mode != 1) throw std::invalid_argument("latent mode must be 0 (exact: R's stream, the reference's draw) or 1 (parallel: counter-based, one thread per observation)");
    if (mode == latMode_) return;
    if (mode == 1 && !binary_) throw std::invalid_argument("latent mode 1 (parallel) draws probit latents: this sampler's response is continuous");
    if (ran_) throw std::invalid_argument("the latent mode is set before the first run");
    if constexpr (kLatentMode) { dev_.set_latent_mode(mode, latKey_); latMode_ = mode; }
    else throw std::invalid_argument("this device layer has no parallel latent draw: latent mode 1 needs the HIP device layer");
  }
  // TEST ENTRY (s4b_test_draw_latents): one latent draw of the sampler's latent mode from the state as it stands (set_state), nothing else of a sweep
  void test_draw_latents() {
    live();
    if (!binary_) throw std::invalid_argument("test_draw_latents: this sampler's response is continuous (no probit latents)");
    if constexpr (has_test_draw_latents<Dev>::value) { dev_.test_draw_latents(); check_device(); }
    else throw std::invalid_argument("test_draw_latents: this device layer has no latent draw on its own");
  }
  int64_t get_trace(int64_t cap, int32_t* out) { live(); return dev_.get_trace(cap, out); }
  void leaf_assignment(int t, int32_t* out) {
    live();
    if (t < 0 || t >= T_) throw std::invalid_argument("tree index out of range");
    HostTrees h; download_trees(h);
    TreeView tv = h.view(t, nc_);
    std::vector<int16_t> list((size_t)nc_); std::vector<int32_t> rank((size_t)nc_, -1);
    PtrArr<int16_t> la(list.data());
    int nl = tv_list_leaves(tv, 0, la);
    for (int i = 0; i < nl; ++i) rank[(size_t)list[(size_t)i]] = i;
    std::vector<uint16_t> leaf(n_);
    dev_.download_leaf_plane(t, leaf.data());
    for (size_t i = 0; i < n_; ++i) out[i] = rank[leaf[i]];
  }
  void profile_sweep(int nSweeps, double out[8]) { live(); if (nSweeps < 1) throw std::invalid_argument("n_sweeps must be >= 1"); dev_.profile_sweep(nSweeps, thin_, out); out[7] = (double)n_; check_device(); }
  // measurement hook: the O(N) sums of one leapfrog on the device at the current draw; out[3] = N, out[4] = SURVEY §8d's
  // algorithmic bytes per evaluation N (8K + 12z + 20), z = non-zeros of Z per row
  void profile_leapfrog(int nEvals, double out[8]) {
    live();
    if (nEvals < 1) throw std::invalid_argument("n_evals must be >= 1");
    const double* cons = row_.data() + 7;
    for (int i = 0; i < 8; ++i) out[i] = 0.0;
    dev_.profile_leapfrog(nEvals, cons + model_->sp.beta_pos(), cons + model_->sp.b_pos(), out);
    const double z = n_ ? (double)nnz_ / (double)n_ : 0.0;
    out[3] = (double)n_; out[4] = (double)n_ * (8.0 * K_ + 12.0 * z + 20.0);
    check_device();
  }
  void nuts_stats(double out[4]) { live(); nuts_->totals(out); }
  void counters(int64_t out[3]) { live(); out[0] = model_->gradEvals; out[1] = treeUpdates_; out[2] = dev_.launches(); }
  Dev& dev() { return dev_; }

  // ---- sweep groups (sweep_group.hpp).  A device layer with batched kernels (DevHip) keeps its membership and arrives inside its own
  // persistent launch; for one without them this class is the member: its sweeps go through the rendezvous of a HostSweepGroup, whose
  // launch runs each member's sweep in turn.
  static constexpr bool kNativeGroup = has_native_sweep_group<Dev>::value;
  ~SamplerCore() { try { leave_group(); } catch (...) {} }
  static SweepGroup* make_group(int device, int maxMembers) {
    if constexpr (kNativeGroup) return Dev::group_create(device, maxMembers);
    else return new HostSweepGroup(device, maxMembers);
  }
  void join_group(SweepGroup* g) {
    if constexpr (kNativeGroup) dev_.join_group(g);
    else {
      if (group_) throw std::invalid_argument("sweep_group_join: the sampler is already in a sweep group");
      if (g->device() != groupDevice_) throw std::invalid_argument("sweep_group_join: the sampler runs on device " + std::to_string(groupDevice_) + ", the group on device " + std::to_string(g->device()));
      g->join(this); group_ = g;
    }
  }
  void leave_group() {
    if constexpr (kNativeGroup) dev_.leave_group();
    else if (group_) { group_->leave(this); group_ = nullptr; }
  }
  // Scope of one run(): waited for by the other members while inside, withdrawn on the way out (return or exception)
  struct GroupRun {
    SamplerCore& c;
    explicit GroupRun(SamplerCore& cc) : c(cc) { if (SweepGroup* g = c.group()) g->enter_run(c.group_member(), c.group_eligible()); }
    ~GroupRun() { if (SweepGroup* g = c.group()) g->exit_run(c.group_member()); }
    GroupRun(const GroupRun&) = delete;
    GroupRun& operator=(const GroupRun&) = delete;
  };

 private:
  SweepGroup* group_ = nullptr;      // (device layers without batched kernels)
  int groupDevice_ = 0;
  SweepGroup* group() { if constexpr (kNativeGroup) return dev_.group_; else return group_; }
  void* group_member() { if constexpr (kNativeGroup) return &dev_; else return this; }
  bool group_eligible() {
    if constexpr (kNativeGroup) return dev_.group_eligible();
    else { int32_t path[2]; dev_.get_tree_path(path); return n_ <= 4096 && (path[0] == 0 || path[0] == 4); }      // (the solo regime of the persistent path)
  }
  // the BART sweeps of one Gibbs iteration and the Stan block's inputs behind them
  void sweep_and_stan_inputs(bool wantTrain, double* train) {
    if constexpr (!kNativeGroup) {
      if (group_) {
        if (!group_eligible()) { dev_.sweep_and_stan_inputs(thin_, stan_mode(), wantTrain, cX_.data(), cZ_.data(), &s0_, train); group_->count_unbatched(thin_); return; }
        for (int k = 0; k < thin_; ++k) {
          GroupJob job; job.member = this; job.run = [](void* m) { static_cast<SamplerCore*>(m)->dev_.sweep(1); };
          group_->arrive(job);
        }
        dev_.stan_inputs(stan_mode(), wantTrain, cX_.data(), cZ_.data(), &s0_, train);
        return;
      }
    }
    dev_.sweep_and_stan_inputs(thin_, stan_mode(), wantTrain, cX_.data(), cZ_.data(), &s0_, train);
  }
  // The Philox key of latent mode 1: a hash of the generator state and Stan seed the chain was created with — nothing is drawn from R's stream,
  // chains with different seeds get different keys
  static uint64_t latent_key(const uint32_t* rstate, uint32_t seed) {
    auto mix = [](uint64_t z) { z += 0x9E3779B97F4A7C15ull; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); };
    uint64_t h = mix(seed);
    for (int i = 0; i < 625; ++i) h = mix(h ^ rstate[i]);
    return h;
  }
  void dev_latent_state(uint64_t ls[2]) { if constexpr (kLatentMode) dev_.latent_state(ls); else ls[0] = ls[1] = 0; }
  void dev_set_latent_state(const uint64_t ls[2]) { if constexpr (kLatentMode) dev_.set_latent_state(ls[0], ls[1]); }
  static constexpr uint32_t STATE_MAGIC = 0x54423453u;   // "S4BT"
  struct Reader {
    const unsigned char* p; size_t n, pos; const char* what = "exported BART state: truncated";
    void get(void* dst, size_t k) { if (k > n || pos > n - k) throw std::invalid_argument(what); if (k) std::memcpy(dst, p + pos, k); pos += k; }
    uint32_t u32() { uint32_t v; get(&v, 4); return v; }
    uint64_t u64() { uint64_t v; get(&v, 8); return v; }
  };
  bool stored_ = false; int64_t nnz_ = 0;
  std::vector<double> weights_;
  void live() const { if (stored_) throw std::invalid_argument("this call needs a live sampler: a stored BART sampler only predicts"); }
  struct HostTrees {
    std::vector<int16_t> var, left, right, parent, na, dep; std::vector<uint16_t> cut; std::vector<double> mu; std::vector<int32_t> cnt, hwm;
    TreeView view(int t, int nc) { size_t o = (size_t)t * nc; return make_tree_view(var.data() + o, cut.data() + o, left.data() + o, right.data() + o, parent.data() + o, nc, na.data(), dep.data()); }
    void alloc(int T, int nc) { size_t m = (size_t)T * nc; na.assign((size_t)nc, 0); dep.assign((size_t)nc, 0); var.assign(m, NODE_FREE); left.assign(m, -1); right.assign(m, -1); parent.assign(m, -1);
                                cut.assign(m, 0); mu.assign(m, 0.0); cnt.assign(m, 0); hwm.assign((size_t)T, 1); }
  };
  // one kept draw = the used node slots of every tree, packed as 16-byte records
  void keep_current_trees() {
    HostTrees h; download_trees(h);
    for (int t = 0; t < T_; ++t) {
      keptTreeStart_.push_back((int64_t)keptNodes_.size());
      const size_t o = (size_t)t * nc_;
      for (int i = 0; i < h.hwm[(size_t)t]; ++i) {
        PackedNode pn; pn.var = h.var[o + i]; pn.cut = h.cut[o + i]; pn.left = h.left[o + i]; pn.right = h.right[o + i]; pn.mu = h.mu[o + i];
        pn.n = pn.var == NODE_LEAF ? h.cnt[o + i] : 0; pn.pad = 0;
        keptNodes_.push_back(pn);
      }
      {   // observation counts of the internal nodes: children before parents
        PackedNode* base = keptNodes_.data() + keptTreeStart_.back();
        TreeView tv = h.view(t, nc_);
        int nd, k; Walker<TreeView> w(tv, 0);
        while (w.next(nd, k)) if (k == 2) base[nd].n = base[base[nd].left].n + base[base[nd].right].n;
      }
    }
    ScaleState sc; dev_.get_scale(sc);
    keptScale_.push_back(sc.min); keptScale_.push_back(sc.range);
  }
  void download_trees(HostTrees& h) { h.alloc(T_, nc_); dev_.download_trees(h.var.data(), h.cut.data(), h.left.data(), h.right.data(), h.parent.data(), h.mu.data(), h.cnt.data(), h.hwm.data()); }

  int stan_mode() const {   // how the Stan offset is formed from the BART fit (reference src/init.cpp:831-839)
    if (hasUserOffset_ && offsetType_ == OFFSET_BART) return 2;      // stanOffset = userOffset
    if (hasUserOffset_ && offsetType_ == OFFSET_DEFAULT) return 3;   // bart fit + userOffset
    return 1;                                                        // bart fit
  }

  // cut points of every predictor: uniform between the column extremes (dbartsControl useQuantiles = FALSE, the default), or
  // from the distinct values (useQuantiles = TRUE; forwarded by bart_args, reference R/stan4bart_fit.R:440-444): with at most
  // n.cuts + 1 distinct values a cut between every two neighbours, otherwise n.cuts cuts at evenly spaced ranks of the sorted
  // distinct values, each half-way between two neighbours.  (dbarts' rule restated: unpinned)  The cut COUNT of a
  // predictor may shrink below n.cuts then.
  void make_cuts(const double* x, bool quantiles) {
    cuts_.resize((size_t)P_);
    for (int j = 0; j < P_; ++j) {
      const double* col = x + (size_t)j * n_;
      int m = numCuts_[(size_t)j];
      if (quantiles) {
        std::vector<double> u(col, col + n_);
        std::sort(u.begin(), u.end());
        u.erase(std::unique(u.begin(), u.end()), u.end());
        const size_t nu = u.size();
        size_t numCuts, step, offset;
        if (m == 0) { numCuts = 0; step = 1; offset = 0; }      // n_cuts = 0 is a legal request: no rule can use the column (nu / numCuts below would divide by zero)
        else if (nu <= (size_t)m + 1) { numCuts = nu - 1; step = 1; offset = 0; }
        else { numCuts = (size_t)m; step = nu / numCuts; offset = step / 2; }
        cuts_[(size_t)j].resize(numCuts);
        for (size_t k = 0; k < numCuts; ++k) {
          const size_t idx = std::min(k * step + offset, nu - 2);
          cuts_[(size_t)j][k] = 0.5 * (u[idx] + u[idx + 1]);
        }
        numCuts_[(size_t)j] = (int32_t)numCuts;
        continue;
      }
      double mn = col[0], mx = col[0];
      for (size_t i = 1; i < n_; ++i) { if (col[i] < mn) mn = col[i]; if (col[i] > mx) mx = col[i]; }
      cuts_[(size_t)j].resize((size_t)m);
      for (int c = 0; c < m; ++c) cuts_[(size_t)j][(size_t)c] = mn + (double)(c + 1) * (mx - mn) / (double)(m + 1);
    }
  }
  // the sigma / row_scale / y rules of s4b_predict_ppd and s4b_predict_loo: under link 0 one finite sigma > 0 per draw of the sampler and of every peer
  // (gathered into `sigma` in pooled order) and a finite row_scale >= 0 (> 0 beside y); every y finite, under link 1 exactly 0 or 1
  void check_responses(const std::string& who, const s4b_summary_in* rw, const double* y, const double* sigma0, const double* const* peerSigma,
                       const double* rowScale, int np, const SamplerCore* const* peers, int64_t S, std::vector<double>& sigma) const {
    const int64_t nT = rw->n_test, own = (int64_t)keptScale_.size() / 2;
    if (rw->link == 0) {
      if (!sigma0) throw std::invalid_argument(who + ": link 0 needs sigma, one value per draw of the sampler");
      if (np > 0 && !peerSigma) throw std::invalid_argument(who + ": link 0 needs peer_sigma, one vector per peer");
      sigma.reserve((size_t)S);
      for (int x = -1; x < np; ++x) {
        const double* sg = x < 0 ? sigma0 : peerSigma[x];
        const std::string whose = x < 0 ? std::string("sigma") : "peer_sigma[" + std::to_string(x) + "]";
        if (!sg) throw std::invalid_argument(who + ": peer " + std::to_string(x) + ": link 0 needs its sigma vector");
        const int64_t ps = x < 0 ? own : (int64_t)peers[x]->keptScale_.size() / 2;
        for (int64_t k = 0; k < ps; ++k) {
          if (!(std::isfinite(sg[k]) && sg[k] > 0.0)) throw std::invalid_argument(who + ": " + whose + " holds " + std::to_string(sg[k]) + " at draw " + std::to_string(k) + " (every sigma must be finite and > 0)");
          sigma.push_back(sg[k]);
        }
      }
      if (rowScale)
        for (int64_t i = 0; i < nT; ++i) {
          const double v = rowScale[i];
          if (!(std::isfinite(v) && v >= 0.0)) throw std::invalid_argument(who + ": row_scale holds " + std::to_string(v) + " at row " + std::to_string(i) + " (finite and >= 0)");
          if (y && v == 0.0) throw std::invalid_argument(who + ": row_scale is 0 at row " + std::to_string(i) + ": with y every row_scale must be > 0");
        }
    }
    if (y)
      for (int64_t i = 0; i < nT; ++i) {
        const double v = y[i];
        if (!std::isfinite(v)) throw std::invalid_argument(who + ": y holds " + std::to_string(v) + " at row " + std::to_string(i) + " (every y must be finite)");
        if (rw->link != 0 && v != 0.0 && v != 1.0) throw std::invalid_argument(who + ": y holds " + std::to_string(v) + " at row " + std::to_string(i) + ": under link 1 every y is 0 or 1");
      }
  }
  // ---- pooling of several samplers' kept draws into one call (s4b_predict_quantiles, s4b_predict_contrast, s4b_predict_ppd)
  // the peer rules, checked before anything is launched: returns the pooled draw count S (this sampler's draws, then the peers')
  int64_t pool_check(const std::string& who, const s4b_summary_in* rw, int np, bool havePeers, const SamplerCore* const* peers, const double* const* peerDenseCoef,
                     const double* const* peerEllCoef) const {
    const int64_t own = (int64_t)keptScale_.size() / 2;
    if (np < 0) throw std::invalid_argument(who + ": negative n_peers");
    if (np > 0 && (!havePeers || !peers)) throw std::invalid_argument(who + ": n_peers > 0 needs peers");
    if (np > 0 && rw->n_dense > 0 && !peerDenseCoef) throw std::invalid_argument(who + ": n_dense > 0 needs peer_dense_coef, one table per peer");
    if (np > 0 && rw->n_ell > 0 && !peerEllCoef) throw std::invalid_argument(who + ": n_ell > 0 needs peer_ell_coef, one table per peer");
    if (own == 0) throw std::invalid_argument(who + ": the sampler holds no kept draws (bart_control.keep_trees, sampling runs)");
    int64_t S = own;
    for (int x = 0; x < np; ++x) {
      const SamplerCore* pc = peers[x];
      const std::string pw = who + ": peer " + std::to_string(x);
      if (!pc) throw std::invalid_argument(pw + " is a NULL sampler");
      if (pc->P_ != P_) throw std::invalid_argument(pw + " has " + std::to_string(pc->P_) + " BART predictors, the sampler " + std::to_string(P_));
      if (pc->T_ != T_) throw std::invalid_argument(pw + " has " + std::to_string(pc->T_) + " trees per draw, the sampler " + std::to_string(T_));
      if (pc->binary_ != binary_) throw std::invalid_argument(pw + (pc->binary_ ? " has a binary response, the sampler a continuous one" : " has a continuous response, the sampler a binary one"));
      for (int j = 0; j < P_; ++j) {
        const std::vector<double>& ca = cuts_[(size_t)j]; const std::vector<double>& cb = pc->cuts_[(size_t)j];
        if (ca.size() != cb.size() || (ca.size() && std::memcmp(ca.data(), cb.data(), ca.size() * 8) != 0))
          throw std::invalid_argument(pw + " has other cut points of predictor " + std::to_string(j) + " than the sampler (the rows are binned once: pooled samplers must share their training predictors)");
      }
      const int64_t ps = (int64_t)pc->keptScale_.size() / 2;
      if (ps == 0) throw std::invalid_argument(pw + " holds no kept draws (bart_control.keep_trees, sampling runs)");
      if (rw->n_dense > 0 && !peerDenseCoef[x]) throw std::invalid_argument(pw + ": n_dense > 0 needs its dense_coef table");
      if (rw->n_ell > 0 && !peerEllCoef[x]) throw std::invalid_argument(pw + ": n_ell > 0 needs its ell_coef table");
      S += ps;
    }
    if (S > 16384) throw std::invalid_argument(who + ": " + std::to_string(S) + " pooled draws, at most 16384 (one row of the sort as doubles in the LDS of a compute unit)");
    return S;
  }
  // the pool itself: this sampler's draws, then the peers' in their order; tree starts rebased onto the concatenated nodes.  `rows` (a summary_call of
  // this sampler alone) is pointed at the pool's storage, which must outlive the device call; without peers it stays as it is.
  struct DrawPool { std::vector<PackedNode> nodes; std::vector<int64_t> treeStart; std::vector<double> scale, denseCoef, ellCoef; };
  void pool_concat(SummaryCall& rows, DrawPool& pool, const s4b_summary_in* rw, const std::vector<uint16_t>& xb, int np, const SamplerCore* const* peers,
                   const double* const* peerDenseCoef, const double* const* peerEllCoef, int64_t S) const {
    if (np <= 0) return;
    const size_t M = (size_t)rw->n_dense, q = rw->n_ell > 0 ? (size_t)rw->n_ell_coef : 0;
    size_t numNodes = keptNodes_.size();
    for (int x = 0; x < np; ++x) numNodes += peers[x]->keptNodes_.size();
    pool.nodes.reserve(numNodes); pool.treeStart.reserve((size_t)S * (size_t)T_); pool.scale.reserve((size_t)S * 2);
    pool.denseCoef.reserve((size_t)S * M); pool.ellCoef.reserve((size_t)S * q);
    for (int x = -1; x < np; ++x) {
      const SamplerCore* pc = x < 0 ? this : peers[x];
      const size_t ps = pc->keptScale_.size() / 2;
      const int64_t base = (int64_t)pool.nodes.size();
      for (int64_t st : pc->keptTreeStart_) pool.treeStart.push_back(st + base);
      pool.nodes.insert(pool.nodes.end(), pc->keptNodes_.begin(), pc->keptNodes_.end());
      pool.scale.insert(pool.scale.end(), pc->keptScale_.begin(), pc->keptScale_.end());
      const double* dc = x < 0 ? rw->dense_coef : peerDenseCoef ? peerDenseCoef[x] : nullptr;
      const double* ec = x < 0 ? rw->ell_coef : peerEllCoef ? peerEllCoef[x] : nullptr;
      if (M) pool.denseCoef.insert(pool.denseCoef.end(), dc, dc + ps * M);
      if (q) pool.ellCoef.insert(pool.ellCoef.end(), ec, ec + ps * q);
      rows.maxDrawNodes = std::max(rows.maxDrawNodes, pc->summary_call(rw, xb, (int64_t)ps).maxDrawNodes);
    }
    rows.nodes = pool.nodes.data(); rows.numNodes = pool.nodes.size(); rows.treeStart = pool.treeStart.data(); rows.scale = pool.scale.data(); rows.S = S;
    if (M) rows.denseCoef = pool.denseCoef.data();
    if (q) rows.ellCoef = pool.ellCoef.data();
  }
  // ---- what s4b_predict_contrast and s4b_predict_groups share: the checks of a s4b_contrast_in and the arms as the device layer takes them
  // the rows, the probs and the scratch limit
  void contrast_check_in(const std::string& who, const s4b_contrast_in* in, int maxWeights) const {
    check_summary_rows(&in->rows, who, maxWeights);
    if (in->n_probs < 0 || in->n_probs > 16) throw std::invalid_argument(who + ": between 0 and 16 probs per call, not " + std::to_string(in->n_probs));
    if (in->n_probs > 0 && !in->probs) throw std::invalid_argument(who + ": NULL probs");
    for (int j = 0; j < in->n_probs; ++j)
      if (!(in->probs[j] >= 0.0 && in->probs[j] <= 1.0)) throw std::invalid_argument(who + ": prob " + std::to_string(in->probs[j]) + " outside [0, 1]");
    if (in->scratch_bytes < 0) throw std::invalid_argument(who + ": negative scratch_bytes");
  }
  // what a ContrastCall points into: it must outlive the device call
  struct ArmsHold { std::vector<uint16_t> xb, xb0; std::vector<int32_t> order, numBase; DrawPool pool; };
  // arm 0's checks, the peer rules, both arms binned with this sampler's cut points, the differing columns, the pool and the tree order of every pooled
  // draw.  twoArms false (predict_groups with one arm, whose arm-0 pointers are all NULL): the rows and the pool alone.  Returns the pooled draws.
  int64_t contrast_arms(const std::string& who, const s4b_contrast_in* in, const SamplerCore* const* peers, bool twoArms, int64_t* info, ContrastCall& c, ArmsHold& h) const {
    const s4b_summary_in* rw = &in->rows;
    const int64_t own = (int64_t)keptScale_.size() / 2, nT = rw->n_test;
    // arm 0: a part of its own only where arm 1 has that part
    if (in->offset0 && !rw->offset) throw std::invalid_argument(who + ": offset0 given, but arm 1 has no offset");
    if (in->dense0 && rw->n_dense == 0) throw std::invalid_argument(who + ": dense0 given, but arm 1 has no dense part (n_dense = 0)");
    if ((in->ell_index0 || in->ell_value0) && rw->n_ell == 0) throw std::invalid_argument(who + ": ell_index0 / ell_value0 given, but arm 1 has no ELL part (n_ell = 0)");
    if (in->ell_index0)
      for (size_t x = 0, m = (size_t)nT * (size_t)rw->n_ell; x < m; ++x)
        if (in->ell_index0[x] < -1 || in->ell_index0[x] >= rw->n_ell_coef)
          throw std::invalid_argument(who + ": ell_index0 " + std::to_string(in->ell_index0[x]) + " outside [-1, " + std::to_string(rw->n_ell_coef) + ")");
    if (in->x_test0)
      for (size_t x = 0, m = (size_t)nT * (size_t)P_; x < m; ++x) if (std::isnan(in->x_test0[x])) throw std::invalid_argument(who + ": x_test0 holds a NaN");
    const int np = in->n_peers;
    const int64_t S = pool_check(who, rw, np, in->peers != nullptr, peers, in->peer_dense_coef, in->peer_ell_coef);
    h.xb.resize((size_t)P_ * (size_t)nT);
    bin_matrix(rw->x_test, (size_t)nT, h.xb);
    // the differing columns: those whose BINS differ in at least one row (two raw values on the same side of every cut do not differ)
    std::vector<int32_t> diff;
    if (in->x_test0) {
      std::vector<uint16_t> all((size_t)P_ * (size_t)nT);
      bin_matrix(in->x_test0, (size_t)nT, all);
      for (int j = 0; j < P_; ++j)
        if (std::memcmp(all.data() + (size_t)j * (size_t)nT, h.xb.data() + (size_t)j * (size_t)nT, (size_t)nT * 2) != 0) diff.push_back(j);
      if (diff.size() > 2) {
        std::string cols;
        for (int32_t j : diff) cols += (cols.empty() ? "" : ", ") + std::to_string(j);
        throw std::invalid_argument(who + ": the arms differ in " + std::to_string(diff.size()) + " BART columns (" + cols + "), at most 2 are supported");
      }
      for (int32_t j : diff) h.xb0.insert(h.xb0.end(), all.begin() + (size_t)j * (size_t)nT, all.begin() + (size_t)(j + 1) * (size_t)nT);
    }
    c.rows = summary_call(rw, h.xb, own); c.rows.info = info;
    c.D = (int)diff.size(); c.vars[0] = c.D > 0 ? diff[0] : -1; c.vars[1] = c.D > 1 ? diff[1] : -1; c.xb0 = h.xb0.data();
    c.offset0 = in->offset0; c.dense0 = in->dense0; c.ellIndex0 = in->ell_index0; c.ellValue0 = in->ell_value0;
    c.Q = in->n_probs; c.probs = in->probs; c.scratchBytes = in->scratch_bytes;
    pool_concat(c.rows, h.pool, rw, h.xb, np, peers, in->peer_dense_coef, in->peer_ell_coef, S);
    if (!twoArms) return S;
    // the tree order of every pooled draw, each sampler's own trees: pd_tree_order with vars = the differing columns (none: nothing is affected)
    if (c.D == 0) {
      h.order.resize((size_t)(S * T_)); h.numBase.assign((size_t)S, T_);
      for (int64_t k = 0; k < S; ++k) for (int t = 0; t < T_; ++t) h.order[(size_t)(k * T_ + t)] = t;
    } else {
      std::vector<int32_t> o, nb;
      for (int x = -1; x < np; ++x) {
        int64_t mx = 0, tot = 0;
        (x < 0 ? this : peers[x])->pd_tree_order(c.D, c.vars, o, nb, mx, tot);
        h.order.insert(h.order.end(), o.begin(), o.end()); h.numBase.insert(h.numBase.end(), nb.begin(), nb.end());
        c.maxAffected = std::max(c.maxAffected, mx); c.totalAffected += tot;
      }
    }
    c.order = h.order.data(); c.numBase = h.numBase.data();
    return S;
  }
  // what s4b_predict_summary and s4b_partial_dependence check of their rows (s4b_summary_in) before anything is launched
  void check_summary_rows(const s4b_summary_in* in, const std::string& who, int maxWeights) const {
    const int64_t nT = in->n_test;
    if (nT < 1 || !in->x_test) throw std::invalid_argument(who + ": x_test must have at least one row");
    if (in->n_weights < 0 || in->n_weights > maxWeights) throw std::invalid_argument(who + ": between 0 and " + std::to_string(maxWeights) + " weight vectors, not " + std::to_string(in->n_weights));
    if (in->link != 0 && in->link != 1) throw std::invalid_argument(who + ": link must be 0 (identity) or 1 (standard normal cdf)");
    if (in->n_dense < 0 || in->n_ell < 0) throw std::invalid_argument(who + ": negative n_dense or n_ell");
    if (in->n_dense > 0 && (!in->dense || !in->dense_coef)) throw std::invalid_argument(who + ": n_dense > 0 needs dense and dense_coef");
    if (in->n_ell > 0 && (!in->ell_index || !in->ell_value || !in->ell_coef || in->n_ell_coef < 1))
      throw std::invalid_argument(who + ": n_ell > 0 needs ell_index, ell_value, ell_coef and n_ell_coef >= 1");
    if (in->n_weights > 0 && !in->weights) throw std::invalid_argument(who + ": n_weights > 0 needs weights");
    if (in->route < 0 || in->route > 2) throw std::invalid_argument(who + ": route must be 0 (automatic), 1 (staged) or 2 (global)");
    if (in->stage_nodes < 0 || in->max_workgroups < 0) throw std::invalid_argument(who + ": negative stage_nodes or max_workgroups");
    for (size_t x = 0, m = (size_t)nT * (size_t)in->n_ell; x < m; ++x)
      if (in->ell_index[x] < -1 || in->ell_index[x] >= in->n_ell_coef)
        throw std::invalid_argument(who + ": ell_index " + std::to_string(in->ell_index[x]) + " outside [-1, " + std::to_string(in->n_ell_coef) + ")");
  }
  // the rows of such a call as the device layer takes them: the kept trees, the largest draw, the validated arguments
  SummaryCall summary_call(const s4b_summary_in* in, const std::vector<uint16_t>& xb, int64_t S) const {
    const int64_t nT = in->n_test;
    int64_t largest = 0;
    for (int64_t k = 0; k < S; ++k) {
      const int64_t en = k + 1 < S ? keptTreeStart_[(size_t)((k + 1) * T_)] : (int64_t)keptNodes_.size();
      largest = std::max(largest, en - keptTreeStart_[(size_t)(k * T_)]);
    }
    SummaryCall c{};
    c.xb = xb.data(); c.nT = nT; c.nodes = keptNodes_.data(); c.numNodes = keptNodes_.size(); c.treeStart = keptTreeStart_.data(); c.S = S; c.T = T_;
    c.scale = keptScale_.data(); c.binary = binary_ ? 1 : 0; c.maxDrawNodes = largest;
    c.offset = in->offset; c.M = in->n_dense; c.dense = in->dense; c.denseCoef = in->dense_coef;
    c.E = in->n_ell; c.q = in->n_ell_coef; c.ellIndex = in->ell_index; c.ellValue = in->ell_value; c.ellCoef = in->ell_coef;
    c.link = in->link; c.G = in->n_weights; c.weights = in->weights; c.route = in->route; c.stageNodes = in->stage_nodes; c.maxWorkgroups = in->max_workgroups;
    return c;
  }
  void bin_matrix(const double* x, size_t m, std::vector<uint16_t>& out) const {
    auto work = [&](int j0, int j1) {
      for (int j = j0; j < j1; ++j) {
        const std::vector<double>& c = cuts_[(size_t)j];
        const double* col = x + (size_t)j * m; uint16_t* o = out.data() + (size_t)j * m;
        for (size_t i = 0; i < m; ++i) o[i] = (uint16_t)(std::lower_bound(c.begin(), c.end(), col[i]) - c.begin());   // #cuts strictly below x
      }
    };
    unsigned nt = std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), (unsigned)P_);
    if ((size_t)P_ * m < (1u << 22)) nt = 1;
    std::vector<std::thread> th;
    for (unsigned k = 0; k < nt; ++k) th.emplace_back(work, (int)((size_t)P_ * k / nt), (int)((size_t)P_ * (k + 1) / nt));
    for (auto& t : th) t.join();
  }

  // dbarts sampleTreesFromPrior (reference src/init.cpp:261): structure by recursive growth, leaf values from the prior
  void grow(TreeView& tv, int& hwm, int node) {
    tv_fill_info_node(tv, hostModelView_, node);
    double pg = tv_growth(tv, hostModelView_, node);
    if (pg <= 0.0) return;
    if (!(r_unif(&rng_) < pg)) return;
    int v = tv_draw_var(tv, hostModelView_, node, &rng_);
    int lo, hi; tv_interval(tv, hostModelView_, node, v, lo, hi);
    int s = r_unif_int(&rng_, lo, hi + 1);
    int L = tv_alloc(tv, hwm); if (L < 0) throw std::runtime_error("node capacity exceeded while sampling trees from the prior");
    tv.var.set(L, NODE_LEAF);
    int R = tv_alloc(tv, hwm); if (R < 0) throw std::runtime_error("node capacity exceeded while sampling trees from the prior");
    tv.var.set(node, (int16_t)v); tv.cut.set(node, (uint16_t)s); tv.left.set(node, (int16_t)L); tv.right.set(node, (int16_t)R);
    tv.var.set(L, NODE_LEAF); tv.parent.set(L, (int16_t)node); tv.left.set(L, -1); tv.right.set(L, -1);
    tv.var.set(R, NODE_LEAF); tv.parent.set(R, (int16_t)node); tv.left.set(R, -1); tv.right.set(R, -1);
    grow(tv, hwm, L); grow(tv, hwm, R);
  }
  void sample_trees_from_prior() {
    HostTrees h; h.alloc(T_, nc_);
    std::vector<int16_t> list((size_t)nc_);
    for (int t = 0; t < T_; ++t) {
      TreeView tv = h.view(t, nc_);
      tv.var.set(0, NODE_LEAF); tv.parent.set(0, -1);
      int hwm = 1;
      grow(tv, hwm, 0);
      PtrArr<int16_t> la(list.data());
      int nl = tv_list_leaves(tv, 0, la);
      for (int i = 0; i < nl; ++i) h.mu[(size_t)t * nc_ + list[(size_t)i]] = r_norm(&rng_) / std::sqrt(hostModelView_.leafPrec);
      h.hwm[(size_t)t] = hwm;
    }
    dev_.upload_trees(h.var.data(), h.cut.data(), h.left.data(), h.right.data(), h.parent.data(), h.mu.data(), h.hwm.data());
    dev_.upload_rng(rng_);
    dev_.assign_leaves_and_residual();
  }

  void var_counts(int32_t* out) {
    HostTrees h; download_trees(h);
    for (int j = 0; j < P_; ++j) out[j] = 0;
    for (int t = 0; t < T_; ++t) { TreeView tv = h.view(t, nc_); int nd, k; Walker<TreeView> w(tv, 0); while (w.next(nd, k)) if (k == 1) ++out[tv.var.get(nd)]; }
  }

  // G = [X Z]'[X Z]: constant over the whole run (hmc_mode 0).  Z'Z is block-sparse (levels of one grouping
  // factor never co-occur), so G is kept in CSR form: a leapfrog costs O(nnz(G)), not O((K+q)^2).
  void build_gram(const s4b_stan_data* sd) {
    const int M = K_ + q_;
    std::vector<int> idx; std::vector<double> val;
    auto row_of = [&](int64_t i) {
      idx.clear(); val.clear();
      for (int k = 0; k < K_; ++k) { idx.push_back(k); val.push_back(sd->X[(size_t)k * sd->N + i]); }
      if (q_) for (int e = sd->u[i]; e < sd->u[i + 1]; ++e) { idx.push_back(K_ + sd->v[e]); val.push_back(sd->w[e]); }
      return weights_.empty() ? 1.0 : weights_[(size_t)i];   // weighted likelihood: G = [X Z]' W [X Z]
    };
    gramPtr_.assign((size_t)M + 1, 0); gramCol_.clear(); gram_.clear();
    if ((size_t)M * (size_t)M <= ((size_t)1 << 22)) {   // small: a dense scratch matrix (32 MB at most), compressed afterwards
      std::vector<double> dense((size_t)M * M, 0.0);
      for (int64_t i = 0; i < sd->N; ++i) {
        const double wi = row_of(i);
        for (size_t a = 0; a < idx.size(); ++a) for (size_t b = 0; b < idx.size(); ++b) dense[(size_t)idx[a] * M + idx[b]] += wi * val[a] * val[b];
      }
      for (int a = 0; a < M; ++a) {
        for (int b = 0; b < M; ++b) if (dense[(size_t)a * M + b] != 0.0) { gramCol_.push_back(b); gram_.push_back(dense[(size_t)a * M + b]); }
        gramPtr_[(size_t)a + 1] = (int)gramCol_.size();
      }
      // a few dozen coefficients whose Gram matrix is mostly filled (crossed grouping factors): rows padded to a multiple of four, so that
      // the matrix-vector product of a leapfrog is straight vector code instead of indexed loads
      gramDense_.clear(); gramLd_ = 0;
      if (M <= 64 && gramCol_.size() * 3 >= (size_t)M * M) {
        gramLd_ = (M + 3) & ~3;
        gramDense_.assign((size_t)M * gramLd_, 0.0);
        for (int a = 0; a < M; ++a) for (int b = 0; b < M; ++b) gramDense_[(size_t)a * gramLd_ + b] = dense[(size_t)a * M + b];
      }
      return;
    }
    // many groups (e.g. a grouping factor with 1e5 levels): G is never formed densely.  Entries are accumulated per (row, column)
    // key in a hash map — a row of [X Z] has K + z non-zeros, so the work is N (K + z)^2 and the memory nnz(G)
    std::unordered_map<uint64_t, double> acc;
    acc.reserve((size_t)sd->N < ((size_t)1 << 22) ? (size_t)sd->N * 4 : ((size_t)1 << 24));
    for (int64_t i = 0; i < sd->N; ++i) {
      const double wi = row_of(i);
      for (size_t a = 0; a < idx.size(); ++a) for (size_t b = 0; b < idx.size(); ++b) acc[(uint64_t)idx[a] * (uint64_t)M + (uint64_t)idx[b]] += wi * val[a] * val[b];
    }
    std::vector<std::pair<uint64_t, double>> ent(acc.begin(), acc.end());
    std::sort(ent.begin(), ent.end(), [](const std::pair<uint64_t, double>& x, const std::pair<uint64_t, double>& y) { return x.first < y.first; });
    for (const auto& e : ent) {
      if (e.second == 0.0) continue;
      const int a = (int)(e.first / (uint64_t)M);
      gramCol_.push_back((int)(e.first % (uint64_t)M)); gram_.push_back(e.second);
      gramPtr_[(size_t)a + 1] = (int)gramCol_.size();
    }
    for (int a = 0; a < M; ++a) if (gramPtr_[(size_t)a + 1] < gramPtr_[(size_t)a]) gramPtr_[(size_t)a + 1] = gramPtr_[(size_t)a];
  }
  // ss = e'We, gX = X'We, gZ = Z'We with e = (y - offset) - X beta - Z b (W = I without weights)
  // A helper thread integrates ahead only where a gradient is closed-form host arithmetic over the Gram form: it never reaches the device layer.
  void sync_runahead() { if (nuts_) nuts_->set_runahead_allowed(model_->has_closed_form() && hmcMode_ == 0 && haveGram_ && model_->gradientCheck == 0); }
  // (th: the calling thread's work space of K + q + 4 doubles, zeros from K + q on; the Gram form reads members only, so two threads may be in it)
  double likelihood(const double* beta, const double* b, double* gX, double* gZ, double* th) {
    if (hmcMode_ != 0) return dev_.leapfrog_sums(beta, b, gX, gZ);
    // (hundreds of calls per Gibbs iteration once the chain runs deep NUTS trees: theta = [beta; b] contiguous, no branch per entry;
    // same products in the same order as the two-array form)
    const int M = K_ + q_;
    for (int k = 0; k < K_; ++k) th[k] = beta[k];
    for (int j = 0; j < q_; ++j) th[K_ + j] = b[j];
    if (gramLd_) {
      return hostloop::gram_dense(host_vector_on(), gramDense_.data(), gramLd_, M, K_, th, cX_.data(), cZ_.data(), s0_, gX, gZ);
    }
    const int* const ptr = gramPtr_.data(); const int* const col = gramCol_.data(); const double* const g = gram_.data();
    double ss = s0_;
    for (int a = 0; a < M; ++a) {
      double ga = 0.0;
      for (int e = ptr[a]; e < ptr[a + 1]; ++e) ga += g[e] * th[col[e]];
      const double ca = a < K_ ? cX_[(size_t)a] : cZ_[(size_t)(a - K_)];
      ss += th[a] * (ga - 2.0 * ca);
      if (a < K_) gX[a] = ca - ga; else gZ[a - K_] = ca - ga;
    }
    return ss;
  }
  void check_device() {
    int32_t e = dev_.error_flags();
    if (e & S4B_ERR_NODE_CAPACITY) throw std::runtime_error("a tree outgrew node_capacity; re-create the sampler with a larger bart_control.node_capacity");
    if (e & S4B_ERR_I_LATENT) throw std::runtime_error("parallel latents: no proposal was accepted for an observation (a mean that is not finite or whose square overflows, |mean| above about 1.3e154; device error word " + std::to_string(e) + ")");
    if (e & S4B_ERR_INTERNAL) throw std::runtime_error("internal error: a hand-shake of the control kernel timed out, or one probit latent needed more than 256 positions of R's stream (device error word " + std::to_string(e) + ")");
    if (e & S4B_ERR_TRACE_OVERFLOW) throw std::runtime_error("trace buffer overflow: call get_trace more often");
  }

  Dev dev_;
  size_t n_ = 0, nTest_ = 0; int P_ = 0, T_ = 0, nc_ = 256, thin_ = 1, K_ = 0, q_ = 0, hmcMode_ = 0; bool haveGram_ = false;
  int warmup_ = 0, verbose_ = 0, refresh_ = 0, offsetType_ = 0; s4b_progress_fn progress_ = nullptr; void* progressUser_ = nullptr; bool keepFits_ = true, hasUserOffset_ = false, binary_ = false;
  std::vector<double> userOffset_;
  s4b_callback_fn callback_ = nullptr; void* callbackUser_ = nullptr;
  MTState rng_;
  std::vector<int32_t> numCuts_; std::vector<std::vector<double>> cuts_; std::vector<double> splitProbs_;
  std::vector<double> pgDepth_, logPg_, log1mPg_, logInt_;
  ModelView hostModelView_;
  std::unique_ptr<HostModel> model_; std::unique_ptr<Nuts> nuts_;
  bool keepTrees_ = false, kModeled_ = false; double kFixed_ = 2.0;
  int latMode_ = 0; uint64_t latKey_ = 0; bool ran_ = false;
  std::vector<PackedNode> keptNodes_; std::vector<int64_t> keptTreeStart_; std::vector<double> keptScale_;
  std::vector<double> row_, cX_, cZ_, gram_, gramDense_; int gramLd_ = 0; std::vector<int> gramPtr_, gramCol_; double s0_ = 0, sigma_ = 1;
  long treeUpdates_ = 0;
};

}  // namespace s4b
#endif
