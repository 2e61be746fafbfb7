// Per-row response curves along one or two BART predictors (s4b_predict_curves; DESIGN.md 5.16): partial dependence's value kept per row,
//     v(i,g,k) = identity or Phi of ( bart(row i with x[vars[w]] := grid[g, w]; draw k) + lin(i,k) ),      c(i,g,k) = v(i,g,k) - v(i,a,k)  (anchor a; none: c = v)
// summarised over the S pooled draws per (row, grid point) — mean, m2, type-7 quantiles — and across the grid per (row, draw): which grid point is the
// highest / lowest (p_max, p_min: exact shares of the draws) and how far the curve ranges, r(i,k) = max_g c - min_g c, summarised over the draws.
// Included by dev_hip.hip inside namespace s4b, LAST, after readout_check.inc: the walk, the staging and the tree order of a partial-dependence call
// are dev_readout.inc's and dev_pd.inc's, the chunked scratch, the draw segments and the LDS sort dev_quantile.inc's, k_level_rows dev_groups.inc's.
//
// THE ORDER OF THE ADDITIONS (include/stan4bart_amd.h states it, tests/curve_cases.py models it) is curve_point's below and nothing else: a value
// depends on its (row, grid point, draw) alone — not on G, the other grid points, the store scheme, the chunking, the route or the kind of sampler.
//   anchor < 0 or link 1:   base = walk_trees(0.0; the unaffected trees, the row's own bins), f_g = walk_trees(base; the affected trees under grid point g),
//                           z_g = response_scale(f_g) + lin (k_partial_dependence's expression), v_g = z_g or readout_phi(z_g), c = v_g - v_a.
//   anchor >= 0, link 0:    s_g = walk_trees(0.0; the affected trees under g), c = range_k (s_g - s_a): k_contrast_values' formula.  The unaffected trees and
//                           the linear parts cancel: not walked, not uploaded.
// Per chunk of C rows (chunk_plan with G values per row and draw: C = scratch / (8 S G) in multiples of 64) the scratch holds the chunk's curves row-major over the pseudo-rows (row, g):
// vals[((r G) + g) S + k], so that k_row_quantiles and k_level_rows run over it UNCHANGED with C G rows.
//   k_curve_values<STAGED, CANCEL>   k_contrast_values' loop (tiles of PS_BLOCK rows, blockIdx.y segments of draws, double-buffered stage_draw<true>) around
//       k_partial_dependence's walk: base once per (row, draw), the affected trees per grid point.
//       THE STORE.  A thread has G values per draw, each bound for an address 8 S bytes from the next; a group of QT_GROUP draws x G points does not fit
//       its registers (PS_BLOCK = 1024 threads leave 128 VGPRs), nor does 1024 rows x G x a group fit the LDS beside the staging buffers.  Every value is
//       stored where it belongs with a plain 8-byte store.  A tile of grid points x a group of draws in registers — whole 64-byte segments, one pass
//       over the segment's draws per tile, base kept between the passes — was built and measured against it: slower or equal at 14 of 16 shapes
//       (DESIGN.md 5.16), so it is not kept.
//       SCALAR REGISTERS.  Four concurrent walks, the staging and some thirty uniform pointers and counts of the argument exceed the 102 SGPRs of a wave:
//       the walking kernels of the family spill some into vector lanes.  Here everything uniform that the walk itself does not read — the tables of the
//       linear parts, the scales, the tree order, the grid's bins, the scratch, the counts of the loop — is moved into vector registers once
//       (cv_vector: an empty asm statement with a VGPR operand), of which a thread has to spare.  No instance spills.
//   k_curve_rows      one workgroup per slab of CV_SLAB rows of the chunk, a wave per row, lanes over the draws: a lane reads its G values (coalesced along
//                     k), keeps max, min and the LOWEST index of each (strict compares in ascending g), stores r(i,k) = max - min into base[r S + k] and
//                     counts its indices in integer LDS counters; lane g then stores count / S.  No floating-point atomics anywhere.
//   k_level_rows, k_row_quantiles   unchanged: over vals as C G levels / rows of unit weight (mean, m2, quantiles), over base as C rows (the range's).
constexpr int64_t CV_SCRATCH_DEFAULT = (int64_t)512 << 20;   // value scratch of a chunk at most: G curves per row make QT_SCRATCH_DEFAULT's 64 MiB a chunk of few tiles (DESIGN.md 5.16)
constexpr int CV_BLOCK = 256;              // threads per workgroup of k_curve_rows
constexpr int CV_SLAB = 64;                // rows per workgroup of k_curve_rows

struct CurvesDev : QuantileDev {
  const int32_t* order; const int32_t* numBase; const uint16_t* gridBin;          // [S x T], [S], [V x G]
  double* base;                                                                   // [C x S]: r(i,k)
  double* pMax; double* pMin;                                                     // [nT x G] each or NULL
  int G, V, var0, var1, anchor;
};

// v(i,g,k) (CANCEL: s_g) of one grid point: the affected trees [nBase, T) of the draw in the call's tree order under grid point g, added to `base`
template <bool STAGED, bool CANCEL>
__device__ __forceinline__ double curve_point(const CurvesDev& a, const WalkNode* lbase, const int32_t* lstart, const int64_t* gstart, const int32_t* ord, int nBase,
                                              size_t ii, int g, double base, double lin, double range, double lo) {
  const int bin0 = a.gridBin[g], bin1 = a.V > 1 ? a.gridBin[a.G + g] : 0;
  const double f = walk_trees<STAGED, true, true>(CANCEL ? 0.0 : base, a, lbase, lstart, gstart, ord, nBase, a.T, ii, a.var0, a.var1, bin0, bin1);
  if (CANCEL) return f;
  const double z = (a.binary ? f : (f + 0.5) * range + lo) + lin;
  return a.link ? readout_phi(z) : z;
}
// c from the point's and the anchor's value
template <bool CANCEL>
__device__ __forceinline__ double curve_centre(const CurvesDev& a, double v, double va, double range) {
  if (a.anchor < 0) return v;
  return CANCEL ? range * (v - va) : v - va;
}

// x as the compiler must keep it in a vector register from here on (a uniform value would else take scalar registers for as long as it lives)
template <class V> __device__ __forceinline__ V cv_vector(V x) { asm("" : "+v"(x)); return x; }

template <bool STAGED, bool CANCEL>
__global__ __launch_bounds__(PS_BLOCK) void k_curve_values(CurvesDev arg) {
  extern __shared__ __align__(16) unsigned char cu_lds[];
  CurvesDev a = arg;
  // what the walk does not read goes to vector registers (the header comment: SCALAR REGISTERS)
  a.scale = cv_vector(a.scale); a.offset = cv_vector(a.offset); a.dense = cv_vector(a.dense); a.denseCoef = cv_vector(a.denseCoef);
  a.ellIndex = cv_vector(a.ellIndex); a.ellValue = cv_vector(a.ellValue); a.ellCoef = cv_vector(a.ellCoef);
  a.numBase = cv_vector(a.numBase); a.gridBin = cv_vector(a.gridBin); a.vals = cv_vector(a.vals);
  a.S = cv_vector(a.S); a.chunk0 = cv_vector(a.chunk0); a.chunkRows = cv_vector(a.chunkRows);
  a.M = cv_vector(a.M); a.E = cv_vector(a.E); a.q = cv_vector(a.q); a.V = cv_vector(a.V); a.var0 = cv_vector(a.var0); a.var1 = cv_vector(a.var1);
  if (STAGED) { a.treeStart = cv_vector(a.treeStart); a.order = cv_vector(a.order); a.numNodes = cv_vector(a.numNodes); }
  WalkNode* nbuf = (WalkNode*)cu_lds;                                              // [2][stageNodes]
  int32_t* sbuf = (int32_t*)(cu_lds + (size_t)2 * a.stageNodes * sizeof(WalkNode));   // [2][2 T]: tree starts inside the draw, then the tree order
  const int tid = threadIdx.x, T = a.T, G = a.G;
  const int64_t S = a.S, C = a.chunkRows;
  const int64_t tiles = (C + PS_BLOCK - 1) / PS_BLOCK;
  auto stage = [&](int64_t k, int b) { stage_draw<true>(a, k, nbuf + (size_t)b * a.stageNodes, sbuf + (size_t)b * 2 * T, a.order); };

  const int64_t k0 = (int64_t)blockIdx.y * a.segDraws, k1 = min(S, k0 + a.segDraws);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r = tile * PS_BLOCK + tid;      // row inside the chunk
    const bool act = r < C;
    const size_t ii = (size_t)(a.chunk0 + (act ? r : C - 1));        // threads beyond the chunk's last row walk that row and store nothing
    const double off = (!CANCEL && a.offset) ? a.offset[ii] : 0.0;
    double* out = a.vals + (size_t)(act ? r : 0) * (size_t)G * (size_t)S;
    __syncthreads();                              // the tile before is done with the staging buffers
    if (STAGED) { stage(k0, 0); __syncthreads(); }
    for (int64_t k = k0; k < k1; ++k) {
      const int b = (int)((k - k0) & 1);
      if (STAGED && k + 1 < k1) stage(k + 1, b ^ 1);          // (last read in draw k - 1, before that draw's barrier)
      const WalkNode* lbase = nbuf + (size_t)b * a.stageNodes;
      const int32_t* lstart = sbuf + (size_t)b * 2 * T;
      const int64_t* gstart = a.treeStart + k * T;
      const int32_t* ord = STAGED ? lstart + T : a.order + k * T;
      const int nBase = __builtin_amdgcn_readfirstlane(a.numBase[k]);          // (the same in every lane: the bounds of the walk stay scalar)
      const double range = a.binary ? 1.0 : a.scale[2 * k + 1], lo = a.binary ? 0.0 : a.scale[2 * k];
      // ---- once per (row, draw): the trees no grid value can move, the linear part at the row's own values, the anchor's value
      double base = 0.0, lin = 0.0, va = 0.0;
      if (!CANCEL) {
        base = walk_trees<STAGED, false, true>(0.0, a, lbase, lstart, gstart, ord, 0, nBase, ii, 0, 0, 0, 0);
        lin = add_linear(off, a, k, ii);
      }
      if (a.anchor >= 0) va = curve_point<STAGED, CANCEL>(a, lbase, lstart, gstart, ord, nBase, ii, a.anchor, base, lin, range, lo);
      // ---- per grid point: the affected trees alone
      for (int g = 0; g < G; ++g) {
        const double v = curve_point<STAGED, CANCEL>(a, lbase, lstart, gstart, ord, nBase, ii, g, base, lin, range, lo);
        if (act) out[(size_t)g * (size_t)S + (size_t)k] = curve_centre<CANCEL>(a, v, va, range);
      }
      if (STAGED) __syncthreads();                // draw k + 1 staged, buffer b free
    }
  }
}

__global__ __launch_bounds__(CV_BLOCK) void k_curve_rows(CurvesDev a) {
  __shared__ int cnt[CV_BLOCK / 64][2][PD_GRID_MAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, G = a.G;
  const int64_t S = a.S, row0 = (int64_t)blockIdx.x * CV_SLAB;                     // first row of the slab inside the chunk
  const int rows = (int)min((int64_t)CV_SLAB, a.chunkRows - row0);
  for (int r0 = 0; r0 < rows; r0 += CV_BLOCK / 64) {                               // (the same trip count for every wave: the barriers below)
    const int r = r0 + wave;
    const bool valid = r < rows;
    cnt[wave][0][lane] = 0; cnt[wave][1][lane] = 0;                                // (PD_GRID_MAX = 64 = the lanes of a wave)
    __syncthreads();
    if (valid) {
      const double* v = a.vals + (size_t)(row0 + r) * (size_t)G * (size_t)S;
      for (int64_t k = lane; k < S; k += 64) {
        double mx = v[k], mn = mx;
        int imx = 0, imn = 0;
        for (int g = 1; g < G; ++g) {                                              // ascending g, strict compares: on an exact tie the lowest index stays
          const double x = v[(size_t)g * (size_t)S + (size_t)k];
          if (x > mx) { mx = x; imx = g; }
          if (x < mn) { mn = x; imn = g; }
        }
        a.base[(size_t)(row0 + r) * (size_t)S + (size_t)k] = mx - mn;
        atomicAdd(&cnt[wave][0][imx], 1); atomicAdd(&cnt[wave][1][imn], 1);        // integer counters in LDS: order-free and exact
      }
    }
    __syncthreads();
    if (valid && lane < G) {
      const size_t x = (size_t)(a.chunk0 + row0 + r) * (size_t)G + (size_t)lane;
      if (a.pMax) a.pMax[x] = (double)cnt[wave][0][lane] / (double)S;
      if (a.pMin) a.pMin[x] = (double)cnt[wave][1][lane] / (double)S;
    }
    __syncthreads();                                                               // the counters are read before the next row clears them
  }
}

template <bool CANCEL>
static void curve_values_launch(hipStream_t stream, const ReadoutPlan& plan, dim3 grid, const CurvesDev& a) {
  if (plan.staged) {
    HIP_OK(hipFuncSetAttribute((const void*)k_curve_values<true, CANCEL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
    hipLaunchKernelGGL((k_curve_values<true, CANCEL>), grid, dim3(PS_BLOCK), plan.lds, stream, a);
  } else hipLaunchKernelGGL((k_curve_values<false, CANCEL>), grid, dim3(PS_BLOCK), 0, stream, a);
}

// uploads, per chunk the value kernel, k_curve_rows and the summary kernels, the downloads — on `stream`, everything allocated here freed here
// (summary_run's discipline)
static void curves_run(hipStream_t stream, int P, const CurvesCall& c, int64_t& launches) {
  SummaryCall r = c.rows;
  const bool cancel = !r.link && c.anchor >= 0;
  const bool walks = !cancel || c.totalAffected > 0;
  if (!walks) r.route = 2;                                        // (nothing to stage)
  if (cancel) { r.offset = nullptr; r.M = 0; r.E = 0; }           // the linear parts cancel: not uploaded, not evaluated
  const ReadoutPlan plan = readout_plan(r, 0, 8, false);          // no reduction space; the workgroups are chosen per chunk
  const ChunkPlan cp = chunk_plan(r.nT, r.S, c.scratchBytes, CV_SCRATCH_DEFAULT, c.G, 64);          // G values per row and draw; Sp and R are a draw row's
  CallBuffers buf(stream);
  const size_t nT = (size_t)r.nT, S = (size_t)r.S, Q = (size_t)c.Q, G = (size_t)c.G;
  const int64_t C = cp.C;
  const bool perPoint = c.mean || c.m2 || Q, extremes = c.pMax || c.pMin || c.rangeMean || c.rangeM2 || c.rangeQuantiles;
  CurvesDev a{};
  buf.upload_rows(a, r, P, plan.stageNodes);
  a.order = buf.alloc(c.order, S * (size_t)r.T);
  a.numBase = buf.alloc(c.numBase, S);
  a.gridBin = buf.alloc(c.gridBin, (size_t)c.V * G);
  a.vals = buf.alloc<double>(nullptr, (size_t)C * G * S);
  a.base = buf.alloc<double>(nullptr, (size_t)C * S);
  if (c.pMax) a.pMax = buf.alloc<double>(nullptr, nT * G);
  if (c.pMin) a.pMin = buf.alloc<double>(nullptr, nT * G);
  a.G = c.G; a.V = c.V; a.var0 = c.vars[0]; a.var1 = c.V > 1 ? c.vars[1] : -2; a.anchor = c.anchor;          // (-2: no node carries it)
  a.Q = c.Q; a.Sp = cp.Sp; a.R = cp.R;
  LevelsSummary sum;          // the chunk's C G curve rows, then its C range rows, as levels of unit weight
  sum.prepare(buf, cp, r.S, c.probs, c.Q, C * c.G);
  double* mean = c.mean ? buf.alloc<double>(nullptr, nT * G) : nullptr;
  double* m2 = c.m2 ? buf.alloc<double>(nullptr, nT * G) : nullptr;
  double* rangeMean = c.rangeMean ? buf.alloc<double>(nullptr, nT) : nullptr;
  double* rangeM2 = c.rangeM2 ? buf.alloc<double>(nullptr, nT) : nullptr;
  double* quantiles = Q ? buf.alloc<double>(nullptr, Q * nT * G) : nullptr;
  double* rangeQuantiles = Q && c.rangeQuantiles ? buf.alloc<double>(nullptr, Q * nT) : nullptr;
  LaunchCount launched{launches};
  for (int64_t ch = 0; ch < cp.chunks; ++ch) {
    a.chunk0 = ch * C; a.chunkRows = std::min<int64_t>(C, r.nT - a.chunk0);
    const dim3 grid = chunk_grid(a);
    if (cancel) curve_values_launch<true>(stream, plan, grid, a); else curve_values_launch<false>(stream, plan, grid, a);
    launched();
    if (perPoint) sum.run(stream, launched, a.vals, a.chunkRows * c.G, a.chunk0 * c.G, mean, m2, quantiles, r.nT * c.G);
    if (extremes) {
      hipLaunchKernelGGL(k_curve_rows, dim3((unsigned)((a.chunkRows + CV_SLAB - 1) / CV_SLAB)), dim3(CV_BLOCK), 0, stream, a); launched();
      if (rangeMean || rangeM2 || rangeQuantiles) sum.run(stream, launched, a.base, a.chunkRows, a.chunk0, rangeMean, rangeM2, rangeQuantiles, r.nT);
    }
  }
  if (mean) HIP_OK(hipMemcpyAsync(c.mean, mean, nT * G * 8, hipMemcpyDeviceToHost, stream));
  if (m2) HIP_OK(hipMemcpyAsync(c.m2, m2, nT * G * 8, hipMemcpyDeviceToHost, stream));
  if (Q) HIP_OK(hipMemcpyAsync(c.quantiles, quantiles, Q * nT * G * 8, hipMemcpyDeviceToHost, stream));
  if (c.pMax) HIP_OK(hipMemcpyAsync(c.pMax, a.pMax, nT * G * 8, hipMemcpyDeviceToHost, stream));
  if (c.pMin) HIP_OK(hipMemcpyAsync(c.pMin, a.pMin, nT * G * 8, hipMemcpyDeviceToHost, stream));
  if (rangeMean) HIP_OK(hipMemcpyAsync(c.rangeMean, rangeMean, nT * 8, hipMemcpyDeviceToHost, stream));
  if (rangeM2) HIP_OK(hipMemcpyAsync(c.rangeM2, rangeM2, nT * 8, hipMemcpyDeviceToHost, stream));
  if (rangeQuantiles) HIP_OK(hipMemcpyAsync(c.rangeQuantiles, rangeQuantiles, Q * nT * 8, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  r.info[0] = !walks ? 0 : plan.staged ? 1 : 2; r.info[1] = C; r.info[2] = cp.chunks; r.info[3] = ((int64_t)cp.R << 32) | (int64_t)cp.Sp;
  r.info[4] = r.maxDrawNodes; r.info[5] = launched.mine; r.info[6] = buf.bytes; r.info[7] = (c.maxAffected << 32) | c.totalAffected;
}
