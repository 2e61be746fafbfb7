// Summaries of the stored-tree predictions, formed on the device WITHOUT the [rows x draws] matrix (s4b_predict_summary; DESIGN.md 5.5).
// Included by dev_hip.hip inside namespace s4b, after k_predict: the walk, the tree order and the scale expression are k_predict's.
//
// For row i and kept draw k
//     z(i,k) = bart(i,k) + offset[i] + sum_j dense[i,j] denseCoef[k,j] + sum_e ellValue[i,e] ellCoef[k, ellIndex[i,e]]      (ellIndex -1: skipped)
//     v(i,k) = z, or Phi(z) under link 1
// and the kernel returns, per row, the mean and the sum of squared deviations of v over the draws (Welford, in draw order, in the thread that owns
// the row) and, per draw, up to PS_GMAX weighted sums over the rows.
//
// Loop structure.  A workgroup owns tiles of PS_BLOCK rows (tile = blockIdx.x, += gridDim.x), one row per thread, and loops over the S draws per tile.
//   STAGED: in front of the walk of draw k every thread copies its share of the nodes of draw k + 1 (16 of PackedNode's 24 bytes: var, cut, left,
//   right, mu) into the other LDS buffer, the tree start offsets beside them; one barrier per draw.  The walk reads a node with one 16-byte LDS read; xb[var * nT + i] stays a global read, coalesced across the rows of a wave.
//   !STAGED: the walk reads PackedNode from global memory as k_predict does (a sampler whose largest draw does not fit the staging buffers).
// Four trees are walked at once per thread (independent chains of dependent loads); their leaf values are added in tree order afterwards, so f is
// k_predict's sum bit for bit.
//
// Per-draw sums: no floating-point atomics.  Every thread forms weights[g,i] * v, a wave adds them with the xor butterfly (fixed pairing), lane 0
// stores the wave's sum in LDS, thread g adds the waves' sums in wave order and adds the result to the workgroup's partial of (draw, g) in global
// memory — only this workgroup touches it, tile after tile.  k_summary_fold adds the workgroups' partials in workgroup order.  Scratch:
// workgroups x S x G doubles.
constexpr int PS_BLOCK = 1024;             // rows per tile = threads per workgroup (16 waves: four per SIMD share one staging)
constexpr int PS_WAVES = PS_BLOCK / 64;
constexpr int PS_GMAX = 8;                 // weight vectors per call
constexpr int PS_STAGE_NODES = 3072;       // nodes per staging buffer at most (48 KB; two buffers)
constexpr int PS_GRID_MAX = 1024;          // workgroups at most (bounds the scratch of the per-draw sums)
constexpr int PS_WALK = 4;                 // trees walked at once per thread
constexpr size_t PS_RED_BYTES = (size_t)2 * PS_WAVES * PS_GMAX * 8;
constexpr size_t PS_LDS_MAX = 160 * 1024;  // LDS of a compute unit (gfx950)

struct alignas(16) WalkNode { int16_t var; uint16_t cut; int16_t left, right; double mu; };
static_assert(sizeof(WalkNode) == 16, "one 16-byte LDS read per node");

struct SummaryDev {          // device pointers of one call
  const uint16_t* xb; const PackedNode* nodes; const int64_t* treeStart; const double* scale;
  const double* offset; const double* dense; const double* denseCoef; const int32_t* ellIndex; const double* ellValue; const double* ellCoef;
  const double* weights; double* mean; double* m2; double* part;
  int64_t nT, S, numNodes;
  int T, binary, M, E, q, link, G, stageNodes;
};

static size_t summary_lds_bytes(bool staged, int stageNodes, int T) {
  return PS_RED_BYTES + (staged ? (size_t)2 * ((size_t)stageNodes * sizeof(WalkNode) + (size_t)T * 4) : 0);
}

__device__ __forceinline__ WalkNode walk_node(const WalkNode& p) { return p; }
__device__ __forceinline__ WalkNode walk_node(const PackedNode& p) { WalkNode w; w.var = p.var; w.cut = p.cut; w.left = p.left; w.right = p.right; w.mu = p.mu; return w; }

template <bool STAGED>
__global__ __launch_bounds__(PS_BLOCK) void k_predict_summary(SummaryDev a) {
  extern __shared__ __align__(16) unsigned char ps_lds[];
  double* red = (double*)ps_lds;                                                   // [2][PS_WAVES][PS_GMAX]
  WalkNode* nbuf = (WalkNode*)(ps_lds + PS_RED_BYTES);                             // [2][stageNodes]
  int32_t* sbuf = (int32_t*)(ps_lds + PS_RED_BYTES + (size_t)2 * a.stageNodes * sizeof(WalkNode));   // [2][T]: tree starts inside the draw
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = a.T;
  const int64_t nT = a.nT, S = a.S;
  const int64_t tiles = (nT + PS_BLOCK - 1) / PS_BLOCK;
  // nodes of draw k: [first, first + count)
  auto draw_first = [&](int64_t k) { return a.treeStart[k * T]; };
  auto draw_count = [&](int64_t k) { return (int)min((int64_t)a.stageNodes, (k + 1 < S ? a.treeStart[(k + 1) * T] : a.numNodes) - a.treeStart[k * T]); };

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i = tile * PS_BLOCK + tid;
    const bool act = i < nT;
    const int64_t ii = act ? i : nT - 1;          // threads beyond the last row walk the last row with weight 0 and store nothing
    const double off = a.offset ? a.offset[ii] : 0.0;
    double mean = 0.0, m2 = 0.0;
    __syncthreads();                              // the tile before is done with both halves of `red` and with the staging buffers
    if (STAGED) {
      const int64_t first = draw_first(0); const int cnt = draw_count(0);
      for (int u = tid; u < cnt; u += PS_BLOCK) nbuf[u] = walk_node(a.nodes[first + u]);
      for (int t = tid; t < T; t += PS_BLOCK) sbuf[t] = (int32_t)(a.treeStart[t] - first);
      __syncthreads();
    }
    for (int64_t k = 0; k < S; ++k) {
      const int b = (int)(k & 1);
      if (STAGED && k + 1 < S) {                  // draw k + 1 into the other buffer (last read in draw k - 1, before that draw's barrier): a wave waits for
        const int64_t first = draw_first(k + 1); const int cnt = draw_count(k + 1);          // its own few loads here while the other waves walk draw k
        WalkNode* dst = nbuf + (size_t)(b ^ 1) * a.stageNodes;
        for (int u = tid; u < cnt; u += PS_BLOCK) dst[u] = walk_node(a.nodes[first + u]);
        for (int t = tid; t < T; t += PS_BLOCK) sbuf[(size_t)(b ^ 1) * T + t] = (int32_t)(a.treeStart[(k + 1) * T + t] - first);
      }
      // ---- the walk: k_predict's, four trees at a time
      const WalkNode* lbase = nbuf + (size_t)b * a.stageNodes;
      const int32_t* lstart = sbuf + (size_t)b * T;
      double f = 0.0;
      for (int t0 = 0; t0 < T; t0 += PS_WALK) {
        WalkNode p[PS_WALK];
        const WalkNode* ls[PS_WALK]; const PackedNode* gs[PS_WALK];
#pragma unroll
        for (int u = 0; u < PS_WALK; ++u) {
          const int t = min(t0 + u, T - 1);
          if (STAGED) { ls[u] = lbase + lstart[t]; p[u] = ls[u][0]; }
          else { gs[u] = a.nodes + a.treeStart[k * T + t]; p[u] = walk_node(gs[u][0]); }
        }
        bool more = true;
        // (states are validated when they are loaded; the step cap is a second guard against a walk that never ends)
        for (int guard = 0; more && guard < 32768; ++guard) {
          more = false;
#pragma unroll
          for (int u = 0; u < PS_WALK; ++u) {
            if (p[u].var >= 0) {
              const int nd = (a.xb[(size_t)p[u].var * (size_t)nT + (size_t)ii] <= p[u].cut) ? p[u].left : p[u].right;
              if (STAGED) p[u] = ls[u][nd]; else p[u] = walk_node(gs[u][nd]);
              more |= p[u].var >= 0;
            }
          }
        }
#pragma unroll
        for (int u = 0; u < PS_WALK; ++u) if (t0 + u < T) f += p[u].mu;
      }
      double z = a.binary ? f : (f + 0.5) * a.scale[2 * k + 1] + a.scale[2 * k];
      if (a.offset) z += off;
      for (int j = 0; j < a.M; ++j) z += a.dense[(size_t)j * (size_t)nT + (size_t)ii] * a.denseCoef[k * a.M + j];
      for (int e = 0; e < a.E; ++e) {
        const int32_t c = a.ellIndex[(size_t)e * (size_t)nT + (size_t)ii];
        if (c >= 0) z += a.ellValue[(size_t)e * (size_t)nT + (size_t)ii] * a.ellCoef[k * a.q + c];
      }
      const double v = a.link ? 0.5 * erfc(-z * 0.70710678118654752440) : z;
      const double d = v - mean;                  // Welford, in draw order
      mean += d / (double)(k + 1);
      m2 += d * (v - mean);
      for (int g = 0; g < a.G; ++g) {             // (the weights are read again per draw: registers go to the walk)
        const double s = wave_sum(act ? a.weights[(size_t)g * (size_t)nT + (size_t)ii] * v : 0.0);
        if (lane == 0) red[((size_t)b * PS_WAVES + wave) * PS_GMAX + g] = s;
      }
      __syncthreads();                            // draw k + 1 staged, the waves' sums of draw k visible, buffer b free
      if (tid < a.G) {
        double s = 0.0;
        for (int wv = 0; wv < PS_WAVES; ++wv) s += red[((size_t)b * PS_WAVES + wv) * PS_GMAX + tid];
        double* dst = a.part + ((size_t)blockIdx.x * (size_t)S + (size_t)k) * (size_t)a.G + tid;
        *dst = (tile == (int64_t)blockIdx.x) ? s : *dst + s;
      }
    }
    if (act) { a.mean[i] = mean; a.m2[i] = m2; }
  }
}

// average[k, g] = the workgroups' partials added in workgroup order
__global__ __launch_bounds__(BLOCK) void k_summary_fold(const double* part, int64_t SG, int workgroups, double* average) {
  for (int64_t x = (int64_t)blockIdx.x * BLOCK + threadIdx.x; x < SG; x += (int64_t)gridDim.x * BLOCK) {
    double s = 0.0;
    for (int wg = 0; wg < workgroups; ++wg) s += part[(size_t)wg * (size_t)SG + (size_t)x];
    average[x] = s;
  }
}

// the route of a call, chosen on the host from the kept trees: staged while the largest draw fits the staging buffers (and they fit the LDS)
struct SummaryPlan { bool staged; int stageNodes; int workgroups; size_t lds; };
static SummaryPlan summary_plan(const SummaryCall& c) {
  SummaryPlan p;
  // the buffers hold what the caller allows (stage_nodes), else the largest draw rounded up to 64 nodes: less LDS where the trees are small
  p.stageNodes = c.stageNodes > 0 ? std::min(c.stageNodes, PS_STAGE_NODES) : (int)std::min<int64_t>(PS_STAGE_NODES, (c.maxDrawNodes + 63) / 64 * 64);
  const bool fits = c.maxDrawNodes <= p.stageNodes && summary_lds_bytes(true, p.stageNodes, c.T) <= PS_LDS_MAX;
  p.staged = c.route != 2 && fits;
  if (!p.staged) p.stageNodes = 0;
  p.lds = summary_lds_bytes(p.staged, p.stageNodes, c.T);
  const int64_t tiles = (c.nT + PS_BLOCK - 1) / PS_BLOCK;
  p.workgroups = (int)std::min<int64_t>(tiles, c.maxWorkgroups > 0 ? std::min(c.maxWorkgroups, PS_GRID_MAX) : PS_GRID_MAX);
  return p;
}

// uploads, the two launches, downloads — on `stream`, everything allocated here freed here (predict_stored's discipline)
static void summary_run(hipStream_t stream, int P, const SummaryCall& c, int64_t& launches) {
  const SummaryPlan plan = summary_plan(c);
  std::vector<void*> held; int64_t bytes = 0;
  auto freeAll = [&] { for (void* q : held) (void)hipFree(q); held.clear(); };
  auto dev = [&](const void* src, size_t n) -> void* {          // a device copy of n host bytes (src NULL: uninitialised)
    void* q = nullptr; const size_t need = std::max<size_t>(16, n);
    HIP_OK(hipMalloc(&q, need)); held.push_back(q); bytes += (int64_t)need;
    if (src && n) HIP_OK(hipMemcpyAsync(q, src, n, hipMemcpyHostToDevice, stream));
    return q;
  };
  try {
    const size_t nT = (size_t)c.nT, S = (size_t)c.S;
    SummaryDev a{};
    a.xb = (const uint16_t*)dev(c.xb, (size_t)P * nT * 2);
    a.nodes = (const PackedNode*)dev(c.nodes, c.numNodes * sizeof(PackedNode));
    a.treeStart = (const int64_t*)dev(c.treeStart, S * (size_t)c.T * 8);
    a.scale = (const double*)dev(c.scale, S * 16);
    a.offset = c.offset ? (const double*)dev(c.offset, nT * 8) : nullptr;
    if (c.M) { a.dense = (const double*)dev(c.dense, nT * (size_t)c.M * 8); a.denseCoef = (const double*)dev(c.denseCoef, S * (size_t)c.M * 8); }
    if (c.E) {
      a.ellIndex = (const int32_t*)dev(c.ellIndex, nT * (size_t)c.E * 4); a.ellValue = (const double*)dev(c.ellValue, nT * (size_t)c.E * 8);
      a.ellCoef = (const double*)dev(c.ellCoef, S * (size_t)c.q * 8);
    }
    double* average = nullptr;
    if (c.G) {
      a.weights = (const double*)dev(c.weights, (size_t)c.G * nT * 8);
      a.part = (double*)dev(nullptr, (size_t)plan.workgroups * S * (size_t)c.G * 8);
      average = (double*)dev(nullptr, S * (size_t)c.G * 8);
    }
    a.mean = (double*)dev(nullptr, nT * 8); a.m2 = (double*)dev(nullptr, nT * 8);
    a.nT = c.nT; a.S = c.S; a.numNodes = (int64_t)c.numNodes; a.T = c.T; a.binary = c.binary; a.M = c.M; a.E = c.E; a.q = c.q; a.link = c.link; a.G = c.G;
    a.stageNodes = plan.stageNodes;
    if (plan.staged) {
      HIP_OK(hipFuncSetAttribute((const void*)k_predict_summary<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
      hipLaunchKernelGGL(k_predict_summary<true>, dim3(plan.workgroups), dim3(PS_BLOCK), plan.lds, stream, a);
    } else hipLaunchKernelGGL(k_predict_summary<false>, dim3(plan.workgroups), dim3(PS_BLOCK), plan.lds, stream, a);
    HIP_OK(hipGetLastError()); ++launches; c.info[5] = 1;
    if (c.G) {
      const int64_t SG = c.S * c.G;
      const int g = (int)std::min<int64_t>(GRID_MAX, (SG + BLOCK - 1) / BLOCK);
      hipLaunchKernelGGL(k_summary_fold, dim3(g), dim3(BLOCK), 0, stream, a.part, SG, plan.workgroups, average);
      HIP_OK(hipGetLastError()); ++launches; c.info[5] = 2;
      HIP_OK(hipMemcpyAsync(c.average, average, (size_t)SG * 8, hipMemcpyDeviceToHost, stream));
    }
    HIP_OK(hipMemcpyAsync(c.mean, a.mean, nT * 8, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(c.m2, a.m2, nT * 8, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    c.info[0] = plan.staged ? 1 : 2; c.info[1] = PS_BLOCK; c.info[2] = plan.workgroups;
    c.info[3] = plan.staged ? (int64_t)((size_t)plan.stageNodes * sizeof(WalkNode) + (size_t)c.T * 4) : 0;
    c.info[4] = c.maxDrawNodes; c.info[6] = bytes; c.info[7] = plan.stageNodes;
  } catch (...) { freeAll(); throw; }
  freeAll();
}
