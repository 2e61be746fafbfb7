// What the read-outs of the kept trees share (DESIGN.md 5.5 - 5.7): s4b_predict_summary (dev_summary.inc), s4b_partial_dependence (dev_pd.inc) and
// s4b_predict_quantiles (dev_quantile.inc).  Included by dev_summary.inc, the first of the three, inside namespace s4b and after k_predict.  The walk,
// the staging of a draw, the linear part, the per-draw reduction, the route and the handling of a call's device buffers exist ONCE, here.
//
// Loop structure of the three walking kernels.  A workgroup owns tiles of PS_BLOCK rows, one row per thread, and loops over draws per tile.
//   STAGED: in front of the walk of draw k every thread copies its share of the nodes of draw k + 1 (16 of PackedNode's 24 bytes: var, cut, left,
//   right, mu) into the other LDS buffer, the tree start offsets (and a tree order) beside them; one barrier per draw, which stays in the kernel.  The
//   walk reads a node with one 16-byte LDS read; xb[var * nT + i] stays a global read, coalesced across the rows of a wave.
//   !STAGED: the walk reads PackedNode from global memory as k_predict does (a sampler whose largest draw does not fit the staging buffers).
// Four trees are walked at once per thread (independent chains of dependent loads); their leaf values are added in the order given afterwards: in
// tree order f is k_predict's sum bit for bit.
//
// Per-draw sums over the rows: no floating-point atomics.  A wave adds its threads' terms with the xor butterfly (fixed pairing), lane 0 stores the
// wave's sum in LDS, after the draw's barrier thread g adds the waves' sums in wave order into the workgroup's partial of (draw, g) in global memory —
// only this workgroup touches it, tile after tile — and k_summary_fold adds the workgroups' partials in workgroup order.
// (PS_BLOCK, PS_STAGE_NODES and PS_WALK are dev_summary.inc's, in front of the include of this file)
constexpr int PS_WAVES = PS_BLOCK / 64;
constexpr int PS_GRID_MAX = 1024;          // workgroups at most (bounds the scratch of the per-draw sums)
constexpr size_t PS_LDS_MAX = 160 * 1024;  // LDS of a compute unit (gfx950)

struct alignas(16) WalkNode { int16_t var; uint16_t cut; int16_t left, right; double mu; };
static_assert(sizeof(WalkNode) == 16, "one 16-byte LDS read per node");
__device__ __forceinline__ WalkNode walk_node(const WalkNode& p) { return p; }
__device__ __forceinline__ WalkNode walk_node(const PackedNode& p) { WalkNode w; w.var = p.var; w.cut = p.cut; w.left = p.left; w.right = p.right; w.mu = p.mu; return w; }

struct RowsDev {             // what every read-out has on the device: the rows, the kept trees, the linear part
  const uint16_t* xb; const PackedNode* nodes; const int64_t* treeStart; const double* scale;
  const double* offset; const double* dense; const double* denseCoef; const int32_t* ellIndex; const double* ellValue; const double* ellCoef;
  int64_t nT, S, numNodes;
  int T, binary, M, E, q, link, stageNodes;
};

// draw k into one staging buffer: its nodes [first, first + count), the tree starts inside the draw and, ORDERED, a tree order behind them.  The caller's
// barrier publishes the buffer.
template <bool ORDERED>
__device__ __forceinline__ void stage_draw(const RowsDev& a, int64_t k, WalkNode* dst, int32_t* sd, const int32_t* order) {
  const int tid = threadIdx.x, T = a.T;
  const int64_t first = a.treeStart[k * T];
  const int cnt = (int)min((int64_t)a.stageNodes, (k + 1 < a.S ? a.treeStart[(k + 1) * T] : a.numNodes) - first);
  for (int u = tid; u < cnt; u += PS_BLOCK) dst[u] = walk_node(a.nodes[first + u]);
  for (int t = tid; t < T; t += PS_BLOCK) { sd[t] = (int32_t)(a.treeStart[k * T + t] - first); if (ORDERED) sd[T + t] = order[k * T + t]; }
}

// the trees [from, to) of one draw for row ii, PS_WALK at a time, their leaf values added to f in that order: trees ord[from .. to) where ORDERED, else
// trees from .. to - 1.  STAGED: tree t starts at lbase + lstart[t], else at a.nodes + gstart[t].  VARY: a node on var0 / var1 takes bin0 / bin1.
template <bool STAGED, bool VARY, bool ORDERED>
__device__ __forceinline__ double walk_trees(double f, const RowsDev& a, const WalkNode* lbase, const int32_t* lstart, const int64_t* gstart, const int32_t* ord,
                                             int from, int to, size_t ii, int var0, int var1, int bin0, int bin1) {
  for (int j0 = from; j0 < to; j0 += PS_WALK) {
    WalkNode p[PS_WALK];
    const WalkNode* ls[PS_WALK]; const PackedNode* gs[PS_WALK];
#pragma unroll
    for (int u = 0; u < PS_WALK; ++u) {
      const int j = min(j0 + u, to - 1), t = ORDERED ? ord[j] : j;
      if (STAGED) { ls[u] = lbase + lstart[t]; p[u] = ls[u][0]; }
      else { gs[u] = a.nodes + gstart[t]; p[u] = walk_node(gs[u][0]); }
    }
    bool more = true;
    // (states are validated when they are loaded; the step cap is a second guard against a walk that never ends)
    for (int guard = 0; more && guard < 32768; ++guard) {
      more = false;
#pragma unroll
      for (int u = 0; u < PS_WALK; ++u) {
        if (p[u].var >= 0) {
          int bin;
          if (VARY && p[u].var == var0) bin = bin0;
          else if (VARY && p[u].var == var1) bin = bin1;
          else bin = a.xb[(size_t)p[u].var * (size_t)a.nT + ii];
          const int nd = (bin <= (int)p[u].cut) ? p[u].left : p[u].right;
          if (STAGED) p[u] = ls[u][nd]; else p[u] = walk_node(gs[u][nd]);
          more |= p[u].var >= 0;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < PS_WALK; ++u) if (j0 + u < to) f += p[u].mu;
  }
  return f;
}
// every tree of draw k in tree order, from 0.0: k_predict's sum
template <bool STAGED>
__device__ __forceinline__ double walk_all(const RowsDev& a, const WalkNode* lbase, const int32_t* lstart, int64_t k, size_t ii) {
  return walk_trees<STAGED, false, false>(0.0, a, lbase, lstart, a.treeStart + k * a.T, nullptr, 0, a.T, ii, 0, 0, 0, 0);
}

// the BART term of draw k on the response scale
__device__ __forceinline__ double response_scale(const RowsDev& a, int64_t k, double f) { return a.binary ? f : (f + 0.5) * a.scale[2 * k + 1] + a.scale[2 * k]; }
// z + sum_j dense[i,j] denseCoef[k,j] + sum_e ellValue[i,e] ellCoef[k, ellIndex[i,e]] (ellIndex -1: skipped), added in that order.  The offset goes in
// front of these terms and stays with the callers: one adds it to a value it has, one starts from it, and 0.0 + offset is not offset where that is -0.0.
__device__ __forceinline__ double add_linear(double z, const RowsDev& a, int64_t k, size_t ii) {
  for (int j = 0; j < a.M; ++j) z += a.dense[(size_t)j * (size_t)a.nT + ii] * a.denseCoef[k * a.M + j];
  for (int e = 0; e < a.E; ++e) {
    const int32_t c = a.ellIndex[(size_t)e * (size_t)a.nT + ii];
    if (c >= 0) z += a.ellValue[(size_t)e * (size_t)a.nT + ii] * a.ellCoef[k * a.q + c];
  }
  return z;
}

// Phi out of line: inlined into a loop that also walks, its thirty-odd polynomial constants are hoisted into registers for the whole kernel and the
// walk spills (DESIGN.md 5.6).  k_predict_summary keeps erfc inline (DESIGN.md 5.5).
__device__ __noinline__ double readout_phi(double z) { return 0.5 * erfc(-z * 0.70710678118654752440); }

// the per-draw reduction, red[2][PS_WAVES][stride] in LDS: the wave's sum of x into column g of half b ...
__device__ __forceinline__ void red_store(double* red, int stride, int b, int g, double x) {
  const double s = wave_sum(x);
  if ((threadIdx.x & 63) == 0) red[((size_t)b * PS_WAVES + (threadIdx.x >> 6)) * stride + g] = s;
}
// ... and, behind the draw's barrier, thread g < G adds the waves in wave order: the workgroup's first tile stores part[(wg * S + k) * G + g], later ones add
__device__ __forceinline__ void red_fold(const double* red, int stride, int b, int G, double* part, int64_t S, int64_t k, bool firstTile) {
  const int g = threadIdx.x;
  if (g < G) {
    double s = 0.0;
    for (int wv = 0; wv < PS_WAVES; ++wv) s += red[((size_t)b * PS_WAVES + wv) * stride + g];
    double* dst = part + ((size_t)blockIdx.x * (size_t)S + (size_t)k) * (size_t)G + g;
    *dst = firstTile ? s : *dst + s;
  }
}
// out[k, g] = the workgroups' partials added in workgroup order
__global__ __launch_bounds__(BLOCK) void k_summary_fold(const double* part, int64_t SG, int workgroups, double* average) {
  for (int64_t x = (int64_t)blockIdx.x * BLOCK + threadIdx.x; x < SG; x += (int64_t)gridDim.x * BLOCK) {
    double s = 0.0;
    for (int wg = 0; wg < workgroups; ++wg) s += part[(size_t)wg * (size_t)SG + (size_t)x];
    average[x] = s;
  }
}
static void fold_partials(hipStream_t stream, const double* part, int64_t SG, int workgroups, double* out, int64_t& launches) {
  const int g = (int)std::min<int64_t>(GRID_MAX, (SG + BLOCK - 1) / BLOCK);
  hipLaunchKernelGGL(k_summary_fold, dim3(g), dim3(BLOCK), 0, stream, part, SG, workgroups, out);
  HIP_OK(hipGetLastError()); ++launches;
}

// the route of a call, chosen on the host from the kept trees: staged while the largest draw fits the staging buffers and they fit the LDS beside the
// kernel's reduction space (redBytes).  A staging buffer holds the nodes and perTreeBytes per tree (4: the tree starts; 8: and a tree order).
struct ReadoutPlan { bool staged; int stageNodes; int workgroups; size_t stageBytes, lds; };          // stageBytes: of one of the two buffers
static ReadoutPlan readout_plan(const SummaryCall& c, size_t redBytes, size_t perTreeBytes, bool wantsWorkgroups) {
  ReadoutPlan p;
  // the buffers hold what the caller allows (stage_nodes), else the largest draw rounded up to 64 nodes: less LDS where the trees are small
  p.stageNodes = c.stageNodes > 0 ? std::min(c.stageNodes, PS_STAGE_NODES) : (int)std::min<int64_t>(PS_STAGE_NODES, (c.maxDrawNodes + 63) / 64 * 64);
  p.stageBytes = (size_t)p.stageNodes * sizeof(WalkNode) + (size_t)c.T * perTreeBytes;
  p.staged = c.route != 2 && c.maxDrawNodes <= p.stageNodes && redBytes + 2 * p.stageBytes <= PS_LDS_MAX;
  if (!p.staged) p.stageNodes = 0, p.stageBytes = 0;
  p.lds = redBytes + 2 * p.stageBytes;
  const int64_t tiles = (c.nT + PS_BLOCK - 1) / PS_BLOCK;
  p.workgroups = !wantsWorkgroups ? 0 : (int)std::min<int64_t>(tiles, c.maxWorkgroups > 0 ? std::min(c.maxWorkgroups, PS_GRID_MAX) : PS_GRID_MAX);
  return p;
}

// the device buffers of one call, on its stream: everything allocated through it is freed when it goes, on a return and on a throw alike
struct CallBuffers {
  hipStream_t stream; std::vector<void*> held; int64_t bytes = 0;
  explicit CallBuffers(hipStream_t s) : stream(s) {}
  CallBuffers(const CallBuffers&) = delete;
  CallBuffers& operator=(const CallBuffers&) = delete;
  ~CallBuffers() { for (void* q : held) (void)hipFree(q); }
  // room for `count` elements, filled from the host where src is given (src NULL: uninitialised)
  template <class V> V* alloc(const V* src, size_t count) {
    const size_t n = count * sizeof(V), need = std::max<size_t>(16, n);
    held.push_back(nullptr);
    HIP_OK(hipMalloc(&held.back(), need)); bytes += (int64_t)need;
    if (src && n) HIP_OK(hipMemcpyAsync(held.back(), src, n, hipMemcpyHostToDevice, stream));
    return (V*)held.back();
  }
  void upload_rows(RowsDev& a, const SummaryCall& c, int P, int stageNodes) {
    const size_t nT = (size_t)c.nT, S = (size_t)c.S;
    a.xb = alloc(c.xb, (size_t)P * nT);
    a.nodes = alloc(c.nodes, c.numNodes);
    a.treeStart = alloc(c.treeStart, S * (size_t)c.T);
    a.scale = alloc(c.scale, S * 2);
    a.offset = c.offset ? alloc(c.offset, nT) : nullptr;
    if (c.M) { a.dense = alloc(c.dense, nT * (size_t)c.M); a.denseCoef = alloc(c.denseCoef, S * (size_t)c.M); }
    if (c.E) { a.ellIndex = alloc(c.ellIndex, nT * (size_t)c.E); a.ellValue = alloc(c.ellValue, nT * (size_t)c.E); a.ellCoef = alloc(c.ellCoef, S * (size_t)c.q); }
    a.nT = c.nT; a.S = c.S; a.numNodes = (int64_t)c.numNodes; a.T = c.T; a.binary = c.binary; a.M = c.M; a.E = c.E; a.q = c.q; a.link = c.link;
    a.stageNodes = stageNodes;
  }
};
