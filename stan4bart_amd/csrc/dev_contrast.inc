// Paired contrasts of two arms over the same rows and the same pooled draws (s4b_predict_contrast; DESIGN.md 5.8): the individual treatment effect
//     d(i,k) = v(z_1(i,k)) - v(z_0(i,k)),      v = identity (link 0) or Phi (link 1)
// summarised on the device: per row mean, sum of squared deviations and type-7 quantiles over the draws, per draw up to PS_GMAX weighted row sums.
// Included by dev_hip.hip inside namespace s4b, after dev_quantile.inc: the walk, the staging, the tree order of a partial-dependence call, the chunked
// value scratch and the LDS sort are dev_readout.inc's, dev_pd.inc's and dev_quantile.inc's.  Shared with the read-outs over one arm or two (dev_groups.inc,
// readout_projection.inc, readout_spread.inc): contrast_rows, contrast_upload and arm_values_prepare / arm_values_launch.
//
// The arms differ in D <= 2 BART columns (found on the host from the BINS of both arms) and in the linear parts whose arm-0 pointer was given.  The
// host orders the trees of every pooled draw as pd_tree_order does with vars = the D columns: unaffected trees first, affected ones behind them.
//   k_contrast_values<STAGED>  k_predict_values' loop (chunk of rows, blockIdx.y segments of draws, QT_GROUP draws stored at once, row-major scratch).
//       link 0: d = range_k (s1 - s0) + (lin1 - lin0); s_a the leaf sum of the AFFECTED trees alone from 0.0 in tree order — arm 1 with the row's
//               own bins, arm 0 with bin0 / bin1 (read once per row from the arm-0 columns) at a node on a differing column; lin_a the linear parts
//               that differ, from the arm's offset (or 0.0) in add_linear's order.  Unaffected trees and shared parts cancel: not evaluated.
//       link 1: base = the unaffected trees once, f_a = base + the affected trees in arm a, z_a = (response_scale(f_a) + shared) + lin_a with `shared`
//               the linear parts that do not differ, formed once; d = readout_phi(z_1) - readout_phi(z_0).  T + A walks where two calls do 2 T.
//       Both arms go through the same code with the same order of additions and d is (arm 1) - (arm 0): swapping the arms negates d bit for bit.
//       The arms of a group of PS_WALK affected trees are walked one after the other: four chains at a time, the registers of k_partial_dependence's
//       walk plus the group of QT_GROUP values (VGPRs: DESIGN.md 5.8).
//   k_contrast_reduce          one workgroup per slab of CT_SLAB rows of the chunk's scratch.  Per row (a wave per row, lanes over the draws, the xor
//                              butterfly): the mean, then sum (d - mean)^2 in a second pass.  Per draw (a thread per draw, the slab's rows in row
//                              order): G weighted sums into part[slab, k, g].  No atomics.
//   k_contrast_fold            average[k, g] += the slabs' partials in slab order (the first chunk starts from 0.0): chunk after chunk.
//   k_row_quantiles            unchanged, on the same scratch, where probs were given.
// The partials of a chunk are ceil(C / CT_SLAB) x S x G doubles with 8 C S <= the value scratch: at most G / CT_SLAB of it, whatever n_test.
constexpr int CT_BLOCK = 256;              // threads per workgroup of k_contrast_reduce
constexpr int CT_SLAB = 64;                // rows per workgroup of k_contrast_reduce

struct ContrastDev : QuantileDev {
  const int32_t* order; const int32_t* numBase;          // [S x T], [S]
  const uint16_t* xb0;                                   // [D x nT]: arm 0's bins of the differing columns
  // arm 0's side of the linear parts that differ, NULL where arm 0 shares arm 1's (dense0 NULL: the dense part is shared; ellIndex0 NULL: the ELL part
  // is shared, else both ellIndex0 and ellValue0 point at what arm 0 uses)
  const double* offset0; const double* dense0; const int32_t* ellIndex0; const double* ellValue0;
  const double* weights; double* mean; double* m2; double* part; double* average;          // [G x nT], [nT], [nT], [slabs x S x G], [S x G]
  int G, D, var0, var1, firstChunk;
};

// z + sum_j dense[i,j] denseCoef[k,j] + sum_e ellValue[i,e] ellCoef[k, ellIndex[i,e]] in add_linear's order, over the row side handed in (a NULL part is left out)
__device__ __forceinline__ double contrast_linear(double z, const RowsDev& a, int64_t k, size_t ii, const double* dense, const int32_t* ellIndex, const double* ellValue) {
  if (dense) for (int j = 0; j < a.M; ++j) z += dense[(size_t)j * (size_t)a.nT + ii] * a.denseCoef[k * a.M + j];
  if (ellIndex) for (int e = 0; e < a.E; ++e) {
    const int32_t c = ellIndex[(size_t)e * (size_t)a.nT + ii];
    if (c >= 0) z += ellValue[(size_t)e * (size_t)a.nT + ii] * a.ellCoef[k * a.q + c];
  }
  return z;
}

template <bool STAGED>
__global__ __launch_bounds__(PS_BLOCK) void k_contrast_values(ContrastDev a) {
  extern __shared__ __align__(16) unsigned char cv_lds[];
  WalkNode* nbuf = (WalkNode*)cv_lds;                                              // [2][stageNodes]
  int32_t* sbuf = (int32_t*)(cv_lds + (size_t)2 * a.stageNodes * sizeof(WalkNode));   // [2][2 T]: tree starts inside the draw, then the tree order
  const int tid = threadIdx.x, T = a.T;
  const int64_t S = a.S, C = a.chunkRows;
  const int64_t tiles = (C + PS_BLOCK - 1) / PS_BLOCK;
  auto stage = [&](int64_t k, int b) { stage_draw<true>(a, k, nbuf + (size_t)b * a.stageNodes, sbuf + (size_t)b * 2 * T, a.order); };

  const int64_t k0 = (int64_t)blockIdx.y * a.segDraws, k1 = min(S, k0 + a.segDraws);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r = tile * PS_BLOCK + tid;      // row inside the chunk
    const bool act = r < C;
    const size_t ii = (size_t)(a.chunk0 + (act ? r : C - 1));        // threads beyond the chunk's last row walk that row and store nothing
    // ---- once per row: arm 0's bins of the differing columns and the offsets
    const int bin0 = a.D > 0 ? a.xb0[ii] : 0, bin1 = a.D > 1 ? a.xb0[(size_t)a.nT + ii] : 0;
    const double off1 = a.offset0 ? a.offset[ii] : 0.0, off0 = a.offset0 ? a.offset0[ii] : 0.0;          // a differing offset, per arm
    const double offShared = (!a.offset0 && a.offset) ? a.offset[ii] : 0.0;                              // link 1 only
    double* out = a.vals + (size_t)(act ? r : 0) * (size_t)S;
    double grp[QT_GROUP];
#pragma unroll
    for (int u = 0; u < QT_GROUP; ++u) grp[u] = 0.0;
    __syncthreads();                              // the tile before is done with the staging buffers
    if (STAGED) { stage(k0, 0); __syncthreads(); }
    for (int64_t k = k0; k < k1; ++k) {
      const int b = (int)((k - k0) & 1);
      if (STAGED && k + 1 < k1) stage(k + 1, b ^ 1);          // (last read in draw k - 1, before that draw's barrier)
      const WalkNode* lbase = nbuf + (size_t)b * a.stageNodes;
      const int32_t* lstart = sbuf + (size_t)b * 2 * T;
      const int64_t* gstart = a.treeStart + k * T;
      const int32_t* ord = STAGED ? lstart + T : a.order + k * T;
      const int nBase = a.numBase[k];
      // the parts of the linear predictor that differ, per arm, through the same code
      const double lin1 = contrast_linear(off1, a, k, ii, a.dense0 ? a.dense : nullptr, a.ellIndex0 ? a.ellIndex : nullptr, a.ellValue);
      const double lin0 = contrast_linear(off0, a, k, ii, a.dense0, a.ellIndex0, a.ellValue0);
      double v;
      if (!a.link) {
        const double s1 = walk_trees<STAGED, false, true>(0.0, a, lbase, lstart, gstart, ord, nBase, T, ii, 0, 0, 0, 0);
        const double s0 = walk_trees<STAGED, true, true>(0.0, a, lbase, lstart, gstart, ord, nBase, T, ii, a.var0, a.var1, bin0, bin1);
        const double range = a.binary ? 1.0 : a.scale[2 * k + 1];
        v = range * (s1 - s0) + (lin1 - lin0);
      } else {
        const double base = walk_trees<STAGED, false, true>(0.0, a, lbase, lstart, gstart, ord, 0, nBase, ii, 0, 0, 0, 0);
        const double f1 = walk_trees<STAGED, false, true>(base, a, lbase, lstart, gstart, ord, nBase, T, ii, 0, 0, 0, 0);
        const double f0 = walk_trees<STAGED, true, true>(base, a, lbase, lstart, gstart, ord, nBase, T, ii, a.var0, a.var1, bin0, bin1);
        const double shared = contrast_linear(offShared, a, k, ii, a.dense0 ? nullptr : a.dense, a.ellIndex0 ? nullptr : a.ellIndex, a.ellValue);
        const double z1 = (response_scale(a, k, f1) + shared) + lin1, z0 = (response_scale(a, k, f0) + shared) + lin0;
        v = readout_phi(z1) - readout_phi(z0);
      }
      // ---- draw k into its place of the group; a full group leaves at once (k_predict_values' stores)
      const int slot = (int)(k % QT_GROUP);
#pragma unroll
      for (int u = 0; u < QT_GROUP; ++u) grp[u] = slot == u ? v : grp[u];
      if (act) {
        if (slot == QT_GROUP - 1) {
          double* dst = out + (k - (QT_GROUP - 1));
#pragma unroll
          for (int u = 0; u < QT_GROUP; ++u) dst[u] = grp[u];
        } else if (k + 1 == k1) {                 // the last, partial group (of the last segment: the others end on a full one)
          double* dst = out + (k - slot);
#pragma unroll
          for (int u = 0; u < QT_GROUP - 1; ++u) if (u <= slot) dst[u] = grp[u];
        }
      }
      if (STAGED) __syncthreads();                // draw k + 1 staged, buffer b free
    }
  }
}

__global__ __launch_bounds__(CT_BLOCK) void k_contrast_reduce(ContrastDev a) {
  const int tid = threadIdx.x;
  const int64_t S = a.S, row0 = (int64_t)blockIdx.x * CT_SLAB;                    // first row of the slab inside the chunk
  const int rows = (int)min((int64_t)CT_SLAB, a.chunkRows - row0);
  const double* slab = a.vals + (size_t)row0 * (size_t)S;
  if (a.mean) {
    const int lane = tid & 63;
    for (int r = tid >> 6; r < rows; r += CT_BLOCK / 64) {
      const double* v = slab + (size_t)r * (size_t)S;
      double s = 0.0;
      for (int64_t k = lane; k < S; k += 64) s += v[k];
      const double mean = wave_sum(s) / (double)S;
      double q = 0.0;
      for (int64_t k = lane; k < S; k += 64) { const double d = v[k] - mean; q += d * d; }
      q = wave_sum(q);
      if (lane == 0) { a.mean[(size_t)(a.chunk0 + row0 + r)] = mean; a.m2[(size_t)(a.chunk0 + row0 + r)] = q; }
    }
  }
  if (a.G) {
    const double* w = a.weights + (size_t)(a.chunk0 + row0);
    for (int64_t k = tid; k < S; k += CT_BLOCK) {
      double acc[PS_GMAX];
#pragma unroll
      for (int g = 0; g < PS_GMAX; ++g) acc[g] = 0.0;
      for (int r = 0; r < rows; ++r) {
        const double v = slab[(size_t)r * (size_t)S + (size_t)k];
#pragma unroll
        for (int g = 0; g < PS_GMAX; ++g) if (g < a.G) acc[g] += w[(size_t)g * (size_t)a.nT + (size_t)r] * v;
      }
      double* dst = a.part + ((size_t)blockIdx.x * (size_t)S + (size_t)k) * (size_t)a.G;
#pragma unroll
      for (int g = 0; g < PS_GMAX; ++g) if (g < a.G) dst[g] = acc[g];
    }
  }
}

// average[x] (+)= the slabs' partials of one chunk in slab order
__global__ __launch_bounds__(BLOCK) void k_contrast_fold(const double* part, int64_t SG, int slabs, double* average, int first) {
  for (int64_t x = (int64_t)blockIdx.x * BLOCK + threadIdx.x; x < SG; x += (int64_t)gridDim.x * BLOCK) {
    double s = first ? 0.0 : average[x];
    for (int b = 0; b < slabs; ++b) s += part[(size_t)b * (size_t)SG + (size_t)x];
    average[x] = s;
  }
}

// the rows of a call as k_contrast_values reads them (shared with dev_groups.inc): `walks` false where no tree is walked
static SummaryCall contrast_rows(const ContrastCall& c, bool& walks) {
  SummaryCall r = c.rows;
  walks = r.link != 0 || c.totalAffected > 0;                     // link 0 without an affected tree: only linear parts are read
  if (!walks) r.route = 2;                                        // (nothing to stage)
  if (!r.link) {                                                  // shared linear parts cancel: not uploaded, not evaluated
    if (!c.offset0) r.offset = nullptr;
    if (!c.dense0) r.M = 0;
    if (!c.ellIndex0 && !c.ellValue0) r.E = 0;
  }
  return r;
}
// what k_contrast_values reads, uploaded: the rows, the tree order, arm 0's side (shared with dev_groups.inc)
static void contrast_upload(CallBuffers& buf, ContrastDev& a, const ContrastCall& c, const SummaryCall& r, int P, const ReadoutPlan& plan) {
  const size_t nT = (size_t)r.nT, S = (size_t)r.S;
  buf.upload_rows(a, r, P, plan.stageNodes);
  a.order = buf.alloc(c.order, S * (size_t)r.T);
  a.numBase = buf.alloc(c.numBase, S);
  if (c.D) a.xb0 = buf.alloc(c.xb0, (size_t)c.D * nT);
  if (c.offset0) a.offset0 = buf.alloc(c.offset0, nT);
  if (c.dense0) a.dense0 = buf.alloc(c.dense0, nT * (size_t)r.M);
  if (c.ellIndex0 || c.ellValue0) {
    a.ellIndex0 = c.ellIndex0 ? buf.alloc(c.ellIndex0, nT * (size_t)r.E) : a.ellIndex;
    a.ellValue0 = c.ellValue0 ? buf.alloc(c.ellValue0, nT * (size_t)r.E) : a.ellValue;
  }
  a.D = c.D; a.var0 = c.D > 0 ? c.vars[0] : -2; a.var1 = c.D > 1 ? c.vars[1] : -2;          // (-2: no node carries it)
}

// the value kernel of a read-out over one arm or two (contrast, groups, projection, spread): k_contrast_values where `two`, else k_predict_values on the
// QuantileDev part of `a` — once per call the LDS of the staged route, then a launch per chunk
static void arm_values_prepare(const ReadoutPlan& plan, bool two) {
  if (!two) return predict_values_prepare(plan);
  if (plan.staged) HIP_OK(hipFuncSetAttribute((const void*)k_contrast_values<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
}
static void arm_values_launch(hipStream_t stream, const ReadoutPlan& plan, dim3 grid, const ContrastDev& a, bool two) {
  if (!two) return predict_values_launch(stream, plan, grid, a);
  if (plan.staged) hipLaunchKernelGGL(k_contrast_values<true>, grid, dim3(PS_BLOCK), plan.lds, stream, a);
  else hipLaunchKernelGGL(k_contrast_values<false>, grid, dim3(PS_BLOCK), 0, stream, a);
}

// uploads, up to four launches per chunk of rows, the downloads — on `stream`, everything allocated here freed here (summary_run's discipline)
static void contrast_run(hipStream_t stream, int P, const ContrastCall& c, int64_t& launches) {
  bool walks;
  SummaryCall r = contrast_rows(c, walks);
  const bool perRow = r.mean != nullptr;
  const ReadoutPlan plan = readout_plan(r, 0, 8, false);          // no reduction space; the workgroups are chosen per chunk
  const ChunkPlan cp = chunk_plan(r.nT, r.S, c.scratchBytes, QT_SCRATCH_DEFAULT, 1, 64);
  CallBuffers buf(stream);
  const size_t nT = (size_t)r.nT, S = (size_t)r.S, Q = (size_t)c.Q, G = (size_t)r.G;
  const int64_t slabsMax = (cp.C + CT_SLAB - 1) / CT_SLAB;
  ContrastDev a{};
  contrast_upload(buf, a, c, r, P, plan);
  a.vals = buf.alloc<double>(nullptr, (size_t)cp.C * S);
  if (perRow) { a.mean = buf.alloc<double>(nullptr, nT); a.m2 = buf.alloc<double>(nullptr, nT); }
  if (G) {
    a.weights = buf.alloc(r.weights, G * nT);
    a.part = buf.alloc<double>(nullptr, (size_t)slabsMax * S * G);
    a.average = buf.alloc<double>(nullptr, S * G);
  }
  if (Q) { a.probs = buf.alloc(c.probs, Q); a.quantiles = buf.alloc<double>(nullptr, Q * nT); }
  a.G = r.G;
  a.Q = c.Q; a.Sp = cp.Sp; a.R = cp.R;
  arm_values_prepare(plan, true);
  if (Q) row_quantiles_prepare(cp);
  LaunchCount launched{launches};
  for (int64_t ch = 0; ch < cp.chunks; ++ch) {
    a.chunk0 = ch * cp.C; a.chunkRows = std::min<int64_t>(cp.C, r.nT - a.chunk0); a.firstChunk = ch == 0;
    arm_values_launch(stream, plan, chunk_grid(a), a, true); launched();
    const int slabs = (int)((a.chunkRows + CT_SLAB - 1) / CT_SLAB);
    if (perRow || G) { hipLaunchKernelGGL(k_contrast_reduce, dim3(slabs), dim3(CT_BLOCK), 0, stream, a); launched(); }
    if (G) {
      const int64_t SG = r.S * r.G;
      const int g = (int)std::min<int64_t>(GRID_MAX, (SG + BLOCK - 1) / BLOCK);
      hipLaunchKernelGGL(k_contrast_fold, dim3(g), dim3(BLOCK), 0, stream, (const double*)a.part, SG, slabs, a.average, a.firstChunk); launched();
    }
    if (Q) { row_quantiles_launch(stream, cp, a); launched(); }
  }
  if (perRow) {
    HIP_OK(hipMemcpyAsync(r.mean, a.mean, nT * 8, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(r.m2, a.m2, nT * 8, hipMemcpyDeviceToHost, stream));
  }
  if (G) HIP_OK(hipMemcpyAsync(r.average, a.average, S * G * 8, hipMemcpyDeviceToHost, stream));
  if (Q) HIP_OK(hipMemcpyAsync(c.quantiles, a.quantiles, Q * nT * 8, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  r.info[0] = !walks ? 0 : plan.staged ? 1 : 2; r.info[1] = cp.C; r.info[2] = cp.chunks; r.info[3] = launched.mine;
  r.info[4] = buf.bytes; r.info[5] = r.S; r.info[6] = c.D; r.info[7] = (c.maxAffected << 32) | c.totalAffected;
}
