// Partial dependence of the kept trees in one fused call (s4b_partial_dependence; DESIGN.md 5.6): dbarts' pdbart / pd2bart on the device.
// Included by dev_hip.hip inside namespace s4b, after dev_summary.inc: WalkNode, walk_node, the tile / draw loop, the staging and the fixed-order
// reduction are k_predict_summary's; k_summary_fold folds the workgroups' partials.
//
// For V = 1 or 2 varied BART predictors vars[w], G <= PD_GRID_MAX grid points (grid point g assigns one value to each varied predictor) and kept draw k
//     pd[k, g] = sum_i weight[i] * v(i, g, k),      v = z or Phi(z),      z = bart(row i with x[vars[w]] := grid[g, w]; draw k) + lin(i, k)
// lin(i, k) = offset[i] + sum_j dense[i,j] denseCoef[k,j] + sum_e ellValue[i,e] ellCoef[k, ellIndex[i,e]] is k_predict_summary's linear part, formed once
// per (i, k) at the rows' OWN values: the varied predictors are BART predictors only, the linear parts do not move with the grid.
//
// A tree without a rule on a varied predictor returns the same leaf for every grid point.  The host orders the trees of every draw — the unaffected
// ones in ascending tree index, then the affected ones in ascending index (order[k, 0 .. T), numBase[k] of them unaffected) — and a thread walks the
// first group once with the row's own bins (`base`) and only the second group per grid point, with bin = gridBin[w, g] at a node on vars[w] and the
// row's own bin elsewhere: T + G * A walks per (row, draw) instead of G * T.  The leaf values are added in that order on both routes, so the BART
// term is NOT k_predict's sum bit for bit (another order of the same T terms), and the staged and the global route agree bit for bit.
//
// Per (draw, g): weight * v through the wave butterfly, lane 0 to LDS (red[2][PS_WAVES][PD_GRID_MAX]: 16 KB), after the draw's barrier thread g adds
// the 16 waves in wave order into the workgroup's partial part[(wg * S + k) * G + g]; k_summary_fold over S * G.  No floating-point atomics.
constexpr int PD_GRID_MAX = 64;            // grid points per call
constexpr size_t PD_RED_BYTES = (size_t)2 * PS_WAVES * PD_GRID_MAX * 8;

struct PdDev {               // device pointers of one call
  const uint16_t* xb; const PackedNode* nodes; const int64_t* treeStart; const double* scale;
  const double* offset; const double* dense; const double* denseCoef; const int32_t* ellIndex; const double* ellValue; const double* ellCoef;
  const double* weight; double* part;
  const int32_t* order; const int32_t* numBase; const uint16_t* gridBin;          // [S x T], [S], [V x G]
  int64_t nT, S, numNodes;
  int T, binary, M, E, q, link, G, V, var0, var1, stageNodes;
};

static size_t pd_lds_bytes(bool staged, int stageNodes, int T) {          // per staging buffer: the nodes, the tree starts and the tree order
  return PD_RED_BYTES + (staged ? (size_t)2 * ((size_t)stageNodes * sizeof(WalkNode) + (size_t)T * 8) : 0);
}

// the trees ord[from .. to) of one draw, four at a time, their leaf values added to f in that order.  VARY: a node on var0 / var1 takes bin0 / bin1.
template <bool STAGED, bool VARY>
__device__ __forceinline__ double pd_walk(double f, const PdDev& a, const WalkNode* lbase, const int32_t* lstart, const int64_t* gstart, const int32_t* ord,
                                          int from, int to, size_t ii, int bin0, int bin1) {
  for (int j0 = from; j0 < to; j0 += PS_WALK) {
    WalkNode p[PS_WALK];
    const WalkNode* ls[PS_WALK]; const PackedNode* gs[PS_WALK];
#pragma unroll
    for (int u = 0; u < PS_WALK; ++u) {
      const int t = ord[min(j0 + u, to - 1)];
      if (STAGED) { ls[u] = lbase + lstart[t]; p[u] = ls[u][0]; }
      else { gs[u] = a.nodes + gstart[t]; p[u] = walk_node(gs[u][0]); }
    }
    bool more = true;
    for (int guard = 0; more && guard < 32768; ++guard) {          // (the step cap: k_predict_summary's second guard)
      more = false;
#pragma unroll
      for (int u = 0; u < PS_WALK; ++u) {
        if (p[u].var >= 0) {
          int bin;
          if (VARY && p[u].var == a.var0) bin = bin0;
          else if (VARY && p[u].var == a.var1) bin = bin1;
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

// Phi out of line: inlined into the grid loop its thirty-odd polynomial constants are hoisted into registers for the whole kernel, and the walk spills
__device__ __noinline__ double pd_phi(double z) { return 0.5 * erfc(-z * 0.70710678118654752440); }

template <bool STAGED>
__global__ __launch_bounds__(PS_BLOCK) void k_partial_dependence(PdDev a) {
  extern __shared__ __align__(16) unsigned char pd_lds[];
  double* red = (double*)pd_lds;                                                   // [2][PS_WAVES][PD_GRID_MAX]
  WalkNode* nbuf = (WalkNode*)(pd_lds + PD_RED_BYTES);                             // [2][stageNodes]
  int32_t* sbuf = (int32_t*)(pd_lds + PD_RED_BYTES + (size_t)2 * a.stageNodes * sizeof(WalkNode));   // [2][2 T]: tree starts inside the draw, then the tree order
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = a.T, G = a.G;
  const int64_t nT = a.nT, S = a.S;
  const int64_t tiles = (nT + PS_BLOCK - 1) / PS_BLOCK;
  auto stage = [&](int64_t k, int b) {           // nodes, tree starts and tree order of draw k into buffer b
    const int64_t first = a.treeStart[k * T];
    const int cnt = (int)min((int64_t)a.stageNodes, (k + 1 < S ? a.treeStart[(k + 1) * T] : a.numNodes) - first);
    WalkNode* dst = nbuf + (size_t)b * a.stageNodes;
    int32_t* sd = sbuf + (size_t)b * 2 * T;
    for (int u = tid; u < cnt; u += PS_BLOCK) dst[u] = walk_node(a.nodes[first + u]);
    for (int t = tid; t < T; t += PS_BLOCK) { sd[t] = (int32_t)(a.treeStart[k * T + t] - first); sd[T + t] = a.order[k * T + t]; }
  };

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i = tile * PS_BLOCK + tid;
    const bool act = i < nT;
    const size_t ii = (size_t)(act ? i : nT - 1);          // threads beyond the last row walk the last row with weight 0
    const double wgt = act ? (a.weight ? a.weight[ii] : 1.0 / (double)nT) : 0.0;
    __syncthreads();                              // the tile before is done with both halves of `red` and with the staging buffers
    if (STAGED) { stage(0, 0); __syncthreads(); }
    for (int64_t k = 0; k < S; ++k) {
      const int b = (int)(k & 1);
      if (STAGED && k + 1 < S) stage(k + 1, b ^ 1);          // (last read in draw k - 1, before that draw's barrier)
      const WalkNode* lbase = nbuf + (size_t)b * a.stageNodes;
      const int32_t* lstart = sbuf + (size_t)b * 2 * T;
      const int64_t* gstart = a.treeStart + k * T;
      const int32_t* ord = STAGED ? lstart + T : a.order + k * T;
      const int nBase = a.numBase[k];
      // ---- once per (row, draw): the trees no grid value can move, and the linear part at the row's own values
      const double base = pd_walk<STAGED, false>(0.0, a, lbase, lstart, gstart, ord, 0, nBase, ii, 0, 0);
      double lin = a.offset ? a.offset[ii] : 0.0;
      for (int j = 0; j < a.M; ++j) lin += a.dense[(size_t)j * (size_t)nT + ii] * a.denseCoef[k * a.M + j];
      for (int e = 0; e < a.E; ++e) {
        const int32_t c = a.ellIndex[(size_t)e * (size_t)nT + ii];
        if (c >= 0) lin += a.ellValue[(size_t)e * (size_t)nT + ii] * a.ellCoef[k * a.q + c];
      }
      const double range = a.binary ? 1.0 : a.scale[2 * k + 1], lo = a.binary ? 0.0 : a.scale[2 * k];
      // ---- per grid point: the affected trees alone
      for (int g = 0; g < G; ++g) {
        const int bin0 = a.gridBin[g], bin1 = a.V > 1 ? a.gridBin[G + g] : 0;
        const double f = pd_walk<STAGED, true>(base, a, lbase, lstart, gstart, ord, nBase, T, ii, bin0, bin1);
        const double z = (a.binary ? f : (f + 0.5) * range + lo) + lin;
        const double v = a.link ? pd_phi(z) : z;
        const double s = wave_sum(wgt * v);
        if (lane == 0) red[((size_t)b * PS_WAVES + wave) * PD_GRID_MAX + g] = s;
      }
      __syncthreads();                            // draw k + 1 staged, the waves' sums of draw k visible, buffer b free
      if (tid < G) {
        double s = 0.0;
        for (int wv = 0; wv < PS_WAVES; ++wv) s += red[((size_t)b * PS_WAVES + wv) * PD_GRID_MAX + tid];
        double* dst = a.part + ((size_t)blockIdx.x * (size_t)S + (size_t)k) * (size_t)G + tid;
        *dst = (tile == (int64_t)blockIdx.x) ? s : *dst + s;
      }
    }
  }
}

// the route of a call: summary_plan's rule with this kernel's LDS (the 16 KB of the reduction and the order table are in the sum)
static SummaryPlan pd_plan(const PdCall& c) {
  const SummaryCall& r = c.rows;
  SummaryPlan p;
  p.stageNodes = r.stageNodes > 0 ? std::min(r.stageNodes, PS_STAGE_NODES) : (int)std::min<int64_t>(PS_STAGE_NODES, (r.maxDrawNodes + 63) / 64 * 64);
  const bool fits = r.maxDrawNodes <= p.stageNodes && pd_lds_bytes(true, p.stageNodes, r.T) <= PS_LDS_MAX;
  p.staged = r.route != 2 && fits;
  if (!p.staged) p.stageNodes = 0;
  p.lds = pd_lds_bytes(p.staged, p.stageNodes, r.T);
  const int64_t tiles = (r.nT + PS_BLOCK - 1) / PS_BLOCK;
  p.workgroups = (int)std::min<int64_t>(tiles, r.maxWorkgroups > 0 ? std::min(r.maxWorkgroups, PS_GRID_MAX) : PS_GRID_MAX);
  return p;
}

// uploads, the two launches, the download — on `stream`, everything allocated here freed here (summary_run's discipline)
static void pd_run(hipStream_t stream, int P, const PdCall& c, int64_t& launches) {
  const SummaryCall& r = c.rows;
  const SummaryPlan plan = pd_plan(c);
  std::vector<void*> held; int64_t bytes = 0;
  auto freeAll = [&] { for (void* q : held) (void)hipFree(q); held.clear(); };
  auto dev = [&](const void* src, size_t n) -> void* {          // a device copy of n host bytes (src NULL: uninitialised)
    void* q = nullptr; const size_t need = std::max<size_t>(16, n);
    HIP_OK(hipMalloc(&q, need)); held.push_back(q); bytes += (int64_t)need;
    if (src && n) HIP_OK(hipMemcpyAsync(q, src, n, hipMemcpyHostToDevice, stream));
    return q;
  };
  try {
    const size_t nT = (size_t)r.nT, S = (size_t)r.S, G = (size_t)c.G;
    PdDev a{};
    a.xb = (const uint16_t*)dev(r.xb, (size_t)P * nT * 2);
    a.nodes = (const PackedNode*)dev(r.nodes, r.numNodes * sizeof(PackedNode));
    a.treeStart = (const int64_t*)dev(r.treeStart, S * (size_t)r.T * 8);
    a.scale = (const double*)dev(r.scale, S * 16);
    a.order = (const int32_t*)dev(c.order, S * (size_t)r.T * 4);
    a.numBase = (const int32_t*)dev(c.numBase, S * 4);
    a.gridBin = (const uint16_t*)dev(c.gridBin, (size_t)c.V * G * 2);
    a.offset = r.offset ? (const double*)dev(r.offset, nT * 8) : nullptr;
    if (r.M) { a.dense = (const double*)dev(r.dense, nT * (size_t)r.M * 8); a.denseCoef = (const double*)dev(r.denseCoef, S * (size_t)r.M * 8); }
    if (r.E) {
      a.ellIndex = (const int32_t*)dev(r.ellIndex, nT * (size_t)r.E * 4); a.ellValue = (const double*)dev(r.ellValue, nT * (size_t)r.E * 8);
      a.ellCoef = (const double*)dev(r.ellCoef, S * (size_t)r.q * 8);
    }
    a.weight = r.weights ? (const double*)dev(r.weights, nT * 8) : nullptr;
    a.part = (double*)dev(nullptr, (size_t)plan.workgroups * S * G * 8);
    double* pd = (double*)dev(nullptr, S * G * 8);
    a.nT = r.nT; a.S = r.S; a.numNodes = (int64_t)r.numNodes; a.T = r.T; a.binary = r.binary; a.M = r.M; a.E = r.E; a.q = r.q; a.link = r.link;
    a.G = c.G; a.V = c.V; a.var0 = c.vars[0]; a.var1 = c.V > 1 ? c.vars[1] : -2;          // (-2: no node carries it)
    a.stageNodes = plan.stageNodes;
    if (plan.staged) {
      HIP_OK(hipFuncSetAttribute((const void*)k_partial_dependence<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
      hipLaunchKernelGGL(k_partial_dependence<true>, dim3(plan.workgroups), dim3(PS_BLOCK), plan.lds, stream, a);
    } else hipLaunchKernelGGL(k_partial_dependence<false>, dim3(plan.workgroups), dim3(PS_BLOCK), plan.lds, stream, a);
    HIP_OK(hipGetLastError()); ++launches; r.info[5] = 1;
    const int64_t SG = r.S * c.G;
    const int fg = (int)std::min<int64_t>(GRID_MAX, (SG + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(k_summary_fold, dim3(fg), dim3(BLOCK), 0, stream, a.part, SG, plan.workgroups, pd);
    HIP_OK(hipGetLastError()); ++launches; r.info[5] = 2;
    HIP_OK(hipMemcpyAsync(c.pd, pd, (size_t)SG * 8, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    r.info[0] = plan.staged ? 1 : 2; r.info[1] = PS_BLOCK; r.info[2] = plan.workgroups;
    r.info[3] = plan.staged ? (int64_t)((size_t)plan.stageNodes * sizeof(WalkNode) + (size_t)r.T * 8) : 0;
    r.info[4] = r.maxDrawNodes; r.info[6] = bytes; r.info[7] = (c.maxAffected << 32) | c.totalAffected;
  } catch (...) { freeAll(); throw; }
  freeAll();
}
