// Partial dependence of the kept trees in one fused call (s4b_partial_dependence; DESIGN.md 5.6): dbarts' pdbart / pd2bart on the device.
// Included by dev_hip.hip inside namespace s4b, after dev_summary.inc and, through it, dev_readout.inc: the walk, the staging, the linear part, the reduction and the route are there.
//
// For V = 1 or 2 varied BART predictors vars[w], G <= PD_GRID_MAX grid points (grid point g assigns one value to each varied predictor) and kept draw k
//     pd[k, g] = sum_i weight[i] * v(i, g, k),      v = z or Phi(z),      z = bart(row i with x[vars[w]] := grid[g, w]; draw k) + lin(i, k)
// lin(i, k) = offset[i] + sum_j dense[i,j] denseCoef[k,j] + sum_e ellValue[i,e] ellCoef[k, ellIndex[i,e]] is formed once per (i, k) at the rows' OWN
// values: the varied predictors are BART predictors only, the linear parts do not move with the grid.
//
// A tree without a rule on a varied predictor returns the same leaf for every grid point.  The host orders the trees of every draw — the unaffected
// ones in ascending tree index, then the affected ones in ascending index (order[k, 0 .. T), numBase[k] of them unaffected) — and a thread walks the
// first group once with the row's own bins (`base`) and only the second group per grid point, with bin = gridBin[w, g] at a node on vars[w] and the
// row's own bin elsewhere: T + G * A walks per (row, draw) instead of G * T.  The leaf values are added in that order on both routes, so the BART
// term is NOT k_predict's sum bit for bit (another order of the same T terms), and the staged and the global route agree bit for bit.
// The reduction's LDS is red[2][PS_WAVES][PD_GRID_MAX]: 16 KB.
constexpr int PD_GRID_MAX = 64;            // grid points per call
constexpr size_t PD_RED_BYTES = (size_t)2 * PS_WAVES * PD_GRID_MAX * 8;

struct PdDev : RowsDev {
  const double* weight; double* part;
  const int32_t* order; const int32_t* numBase; const uint16_t* gridBin;          // [S x T], [S], [V x G]
  int G, V, var0, var1;
};

template <bool STAGED>
__global__ __launch_bounds__(PS_BLOCK) void k_partial_dependence(PdDev a) {
  extern __shared__ __align__(16) unsigned char pd_lds[];
  double* red = (double*)pd_lds;                                                   // [2][PS_WAVES][PD_GRID_MAX]
  WalkNode* nbuf = (WalkNode*)(pd_lds + PD_RED_BYTES);                             // [2][stageNodes]
  int32_t* sbuf = (int32_t*)(pd_lds + PD_RED_BYTES + (size_t)2 * a.stageNodes * sizeof(WalkNode));   // [2][2 T]: tree starts inside the draw, then the tree order
  const int tid = threadIdx.x, T = a.T, G = a.G;
  const int64_t nT = a.nT, S = a.S;
  const int64_t tiles = (nT + PS_BLOCK - 1) / PS_BLOCK;
  auto stage = [&](int64_t k, int b) { stage_draw<true>(a, k, nbuf + (size_t)b * a.stageNodes, sbuf + (size_t)b * 2 * T, a.order); };

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
      const double base = walk_trees<STAGED, false, true>(0.0, a, lbase, lstart, gstart, ord, 0, nBase, ii, 0, 0, 0, 0);
      const double lin = add_linear(a.offset ? a.offset[ii] : 0.0, a, k, ii);
      const double range = a.binary ? 1.0 : a.scale[2 * k + 1], lo = a.binary ? 0.0 : a.scale[2 * k];
      // ---- per grid point: the affected trees alone
      for (int g = 0; g < G; ++g) {
        const int bin0 = a.gridBin[g], bin1 = a.V > 1 ? a.gridBin[G + g] : 0;
        const double f = walk_trees<STAGED, true, true>(base, a, lbase, lstart, gstart, ord, nBase, T, ii, a.var0, a.var1, bin0, bin1);
        const double z = (a.binary ? f : (f + 0.5) * range + lo) + lin;
        red_store(red, PD_GRID_MAX, b, g, wgt * (a.link ? readout_phi(z) : z));
      }
      __syncthreads();                            // draw k + 1 staged, the waves' sums of draw k visible, buffer b free
      red_fold(red, PD_GRID_MAX, b, G, a.part, S, k, tile == (int64_t)blockIdx.x);
    }
  }
}

// uploads, the two launches, the download — on `stream`, everything allocated here freed here (summary_run's discipline)
static void pd_run(hipStream_t stream, int P, const PdCall& c, int64_t& launches) {
  const SummaryCall& r = c.rows;
  const ReadoutPlan plan = readout_plan(r, PD_RED_BYTES, 8, true);
  CallBuffers buf(stream);
  const size_t nT = (size_t)r.nT, S = (size_t)r.S, G = (size_t)c.G;
  PdDev a{};
  buf.upload_rows(a, r, P, plan.stageNodes);
  a.order = buf.alloc(c.order, S * (size_t)r.T);
  a.numBase = buf.alloc(c.numBase, S);
  a.gridBin = buf.alloc(c.gridBin, (size_t)c.V * G);
  a.weight = r.weights ? buf.alloc(r.weights, nT) : nullptr;
  a.part = buf.alloc<double>(nullptr, (size_t)plan.workgroups * S * G);
  double* pd = buf.alloc<double>(nullptr, S * G);
  a.G = c.G; a.V = c.V; a.var0 = c.vars[0]; a.var1 = c.V > 1 ? c.vars[1] : -2;          // (-2: no node carries it)
  if (plan.staged) {
    HIP_OK(hipFuncSetAttribute((const void*)k_partial_dependence<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
    hipLaunchKernelGGL(k_partial_dependence<true>, dim3(plan.workgroups), dim3(PS_BLOCK), plan.lds, stream, a);
  } else hipLaunchKernelGGL(k_partial_dependence<false>, dim3(plan.workgroups), dim3(PS_BLOCK), plan.lds, stream, a);
  HIP_OK(hipGetLastError()); ++launches; r.info[5] = 1;
  fold_partials(stream, a.part, r.S * c.G, plan.workgroups, pd, launches); r.info[5] = 2;
  HIP_OK(hipMemcpyAsync(c.pd, pd, S * G * 8, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  r.info[0] = plan.staged ? 1 : 2; r.info[1] = PS_BLOCK; r.info[2] = plan.workgroups; r.info[3] = (int64_t)plan.stageBytes;
  r.info[4] = r.maxDrawNodes; r.info[6] = buf.bytes; r.info[7] = (c.maxAffected << 32) | c.totalAffected;
}
