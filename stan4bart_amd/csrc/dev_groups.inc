// Per-level sums and means of the rows' values per pooled draw, summarised over the draws (s4b_predict_groups; DESIGN.md 5.12): for rows i with the
// non-decreasing level[i] in [0, L) and weights w_i >= 0
//     a(l,k) = sum_{i : level[i] = l} w_i x(i,k),     x = k_predict_values' v (one arm) or k_contrast_values' d (two arms),
//     A(l,k) = a(l,k) (statistic 0) or a(l,k) / W_l (statistic 1),
// and per level the mean, m2 and type-7 quantiles of A(l, .) and the share of the draws above a threshold.
// Included by dev_hip.hip inside namespace s4b, LAST, after dev_contrast.inc: the value kernels, the chunked scratch, the LDS sort and the call
// scaffold are dev_readout.inc's, dev_quantile.inc's and dev_contrast.inc's.  New here is the segmented reduction over the rows by level.  Shared with
// the read-outs behind it (projection, spread, check, curves): k_level_rows and LevelsSummary, the summary over the draws of a matrix of unit-weight levels.
//
// THE ORDER OF THE ADDITIONS (include/stan4bart_amd.h states it, tests/group_cases.py models it): slabs are the GLOBAL blocks of GP_SLAB rows — a chunk
// starts on a multiple of GP_SLAB, so a slab never depends on the chunking.  a(l,k) is the left fold, over the slabs in ascending order, of the slab's
// partial; a partial is the left fold, over the level's rows of the slab in row order, of w_i x(i,k); the first term of a fold is taken as it is.
// Per chunk of C rows (chunk_plan):
//   k_predict_values<STAGED> / k_contrast_values<STAGED>   unchanged: the chunk's values row-major in the scratch.
//   k_level_reduce    one workgroup (a wave) per slab and segment of GP_BLOCK draws, a draw per thread: vals[r S + k] is read coalesced across the wave,
//                     level[r] and w[r] are the same for every lane (scalar loads).  A thread runs down the slab's rows and closes a partial whenever
//                     the label changes.  A level that lies inside the slab is stored straight into lev[l S + k]; the run at the slab's first row
//                     whose level comes over from the slab before goes to the slab's head partial, else the run at its last row whose level goes on in
//                     the next slab to its tail partial: edge[slab][2][S].  Every address has one writer.
//   k_level_fold      for every level of the chunk that touches more than one slab, a thread per (level, draw): the level's partials in slab order —
//                     from the tail partial of its first slab where that lies in this chunk, else from the running lev[l S + k] of the chunk before,
//                     then the head partials of its further slabs.
// After the last chunk:
//   k_level_rows      a wave per level, lanes over the draws: A in place (the division, or NaN for a level without rows or with W_l = 0 under statistic
//                     1), the mean, sum (A - mean)^2 in a second pass (k_contrast_reduce's per-row arithmetic) and the count above the threshold.
//   k_row_quantiles   unchanged, over the level matrix as its rows, in pieces of at most GP_SORT_LEVELS levels.
// No floating-point atomics, no data-dependent order.  Device memory beyond the value kernel's: edge (2 / GP_SLAB of the scratch), the level matrix
// 8 L S, the labels, the weights, the level starts and the per-level outputs.
constexpr int GP_SLAB = 64;                      // rows per slab: the unit of the fold, part of the interface
constexpr int GP_BLOCK = 64;                     // threads per workgroup of k_level_reduce: one wave, a draw per lane
constexpr int64_t GP_SORT_LEVELS = 1 << 20;      // levels per launch of k_row_quantiles at most

struct GroupsDev {
  const double* vals; const int32_t* level; const double* w;                       // [C x S], [nT], [nT] or NULL (every weight 1)
  double* lev; double* edge;                                                       // [L x S], [slabs of a chunk][2][S]
  const int64_t* levelStart; const double* levelWeight; const int32_t* edgeLevel;  // [L + 1], [L], the levels touching more than one slab, ascending
  double* mean; double* m2; double* pAbove;                                        // [L] each or NULL
  int64_t nT, S, L, chunk0, chunkRows;
  int statistic, hasThreshold; double threshold;
};

__global__ __launch_bounds__(GP_BLOCK) void k_level_reduce(GroupsDev a) {
  const int64_t S = a.S, k = (int64_t)blockIdx.y * GP_BLOCK + threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * GP_SLAB, g0 = a.chunk0 + row0;        // the slab's first row inside the chunk and among all rows
  const int rows = (int)min((int64_t)GP_SLAB, a.chunkRows - row0);
  if (k >= S) return;
  const int32_t* __restrict__ lab = a.level + g0;
  const double* __restrict__ w = a.w ? a.w + g0 : nullptr;
  const double* __restrict__ v = a.vals + (size_t)row0 * (size_t)S + (size_t)k;
  double* edge = a.edge + (size_t)blockIdx.x * 2 * (size_t)S + (size_t)k;
  const bool fromPrev = g0 > 0 && a.level[g0 - 1] == lab[0];                       // the first run's level has rows in the slab before
  const bool toNext = g0 + rows < a.nT && a.level[g0 + rows] == lab[rows - 1];     // the last run's level has rows in the next slab
  int cur = lab[0];
  bool first = true;                                                               // the open run holds the slab's first row
  double acc = w ? w[0] * v[0] : v[0];
  for (int r = 1; r < rows; ++r) {
    const int l = lab[r];
    const double x = w ? w[r] * v[(size_t)r * (size_t)S] : v[(size_t)r * (size_t)S];
    if (l != cur) {                                                                // (the same for every lane)
      if (first && fromPrev) edge[0] = acc; else a.lev[(size_t)cur * (size_t)S + (size_t)k] = acc;
      first = false; cur = l; acc = x;
    } else acc += x;
  }
  if (first && fromPrev) edge[0] = acc;
  else if (toNext) edge[S] = acc;
  else a.lev[(size_t)cur * (size_t)S + (size_t)k] = acc;
}

// the levels edgeLevel[e0 .. e0 + nE) are those of this chunk that touch more than one slab
__global__ __launch_bounds__(BLOCK) void k_level_fold(GroupsDev a, int64_t e0, int64_t nE) {
  const int64_t S = a.S, slab0 = a.chunk0 / GP_SLAB, slab1 = slab0 + (a.chunkRows + GP_SLAB - 1) / GP_SLAB;          // the chunk's slabs [slab0, slab1)
  for (int64_t x = (int64_t)blockIdx.x * BLOCK + threadIdx.x; x < nE * S; x += (int64_t)gridDim.x * BLOCK) {
    const int64_t j = x / S, k = x - j * S;
    const int64_t l = a.edgeLevel[e0 + j];
    const int64_t sb = a.levelStart[l] / GP_SLAB, last = min((a.levelStart[l + 1] - 1) / GP_SLAB, slab1 - 1);
    double* dst = a.lev + (size_t)l * (size_t)S + (size_t)k;
    int64_t s = max(sb, slab0);
    double acc;
    if (sb >= slab0) { acc = a.edge[(size_t)((s - slab0) * 2 + 1) * (size_t)S + (size_t)k]; ++s; }          // the level begins in this chunk: its tail partial as it is
    else acc = *dst;                                                                                          // what the chunk before left
    for (; s <= last; ++s) acc += a.edge[(size_t)((s - slab0) * 2) * (size_t)S + (size_t)k];
    *dst = acc;
  }
}

__global__ __launch_bounds__(BLOCK) void k_level_rows(GroupsDev a) {
  const int lane = threadIdx.x & 63;
  const int64_t S = a.S;
  for (int64_t l = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); l < a.L; l += (int64_t)gridDim.x * (BLOCK / 64)) {
    double* v = a.lev + (size_t)l * (size_t)S;
    const double W = a.levelWeight[l];
    const bool none = a.levelStart[l + 1] == a.levelStart[l] || (a.statistic == 1 && W == 0.0);          // (the same for every lane)
    if (none || a.statistic == 1)
      for (int64_t k = lane; k < S; k += 64) v[k] = none ? __longlong_as_double(0x7ff8000000000000ll) : v[k] / W;          // (read back below by the lane that wrote it)
    double s = 0.0;
    for (int64_t k = lane; k < S; k += 64) s += v[k];
    const double mean = wave_sum(s) / (double)S;
    double q = 0.0, above = 0.0;
    for (int64_t k = lane; k < S; k += 64) { const double d = v[k] - mean; q += d * d; above += (a.hasThreshold && v[k] > a.threshold) ? 1.0 : 0.0; }
    q = wave_sum(q); above = wave_sum(above);                                      // (counts of at most 16 384: exact)
    if (lane == 0) {
      if (a.mean) a.mean[l] = mean;
      if (a.m2) a.m2[l] = q;
      if (a.pAbove) a.pAbove[l] = none ? mean : above / (double)S;
    }
  }
}

// The summary over the draws of a device matrix [n x S] whose rows are levels (groups: its level matrix; projection, spread, check, curves: a matrix
// of statistics or values whose every row is a level of ONE row and unit weight, statistic 0): per row the mean and m2 through k_level_rows and the
// type-7 quantiles through k_row_quantiles, in pieces of at most GP_SORT_LEVELS rows, written at a row offset of the outputs.
struct LevelsSummary {
  std::vector<int64_t> start; std::vector<double> ones;          // the host side of the unit tables: the uploads read it until the call has synchronised
  GroupsDev g{};                                                 // the unit tables of a piece (levelStart 0, 1, 2, ...; levelWeight 1), S, statistic 0, no threshold
  QuantileDev qd{};                                              // the probs, S, Q, Sp, R
  ChunkPlan cp{};
  // once per call: the probs (Q > 0) uploaded and the sort prepared; unitRows > 0: the unit tables for pieces of at most that many rows uploaded
  void prepare(CallBuffers& buf, const ChunkPlan& plan, int64_t S, const double* probs, int Q, int64_t unitRows) {
    cp = plan;
    g.S = S;
    if (unitRows > 0) {
      const size_t piece = (size_t)std::min<int64_t>(GP_SORT_LEVELS, unitRows);
      start.resize(piece + 1);
      for (size_t l = 0; l <= piece; ++l) start[l] = (int64_t)l;
      ones.assign(piece, 1.0);
      g.levelStart = buf.alloc(start.data(), piece + 1); g.levelWeight = buf.alloc(ones.data(), piece);
    }
    if (Q) {
      qd.probs = buf.alloc(probs, (size_t)Q); qd.S = S; qd.Q = Q; qd.Sp = plan.Sp; qd.R = plan.R;
      row_quantiles_prepare(plan);
    }
  }
  // the n rows of vals [n x S] into rows [first, first + n) of the device outputs mean, m2 [total] and quantiles [Q x total], each where not NULL
  void run(hipStream_t stream, LaunchCount& launched, double* vals, int64_t n, int64_t first, double* mean, double* m2, double* quantiles, int64_t total) {
    qd.quantiles = quantiles; qd.nT = total;
    for (int64_t l0 = 0; l0 < n; l0 += GP_SORT_LEVELS) {
      const int64_t L = std::min<int64_t>(GP_SORT_LEVELS, n - l0);
      if (mean || m2) {
        g.lev = vals + (size_t)l0 * (size_t)g.S; g.L = L; g.mean = mean ? mean + first + l0 : nullptr; g.m2 = m2 ? m2 + first + l0 : nullptr;
        hipLaunchKernelGGL(k_level_rows, dim3((unsigned)std::min<int64_t>(GRID_MAX, (L + BLOCK / 64 - 1) / (BLOCK / 64))), dim3(BLOCK), 0, stream, g); launched();
      }
      if (quantiles) {
        qd.vals = vals + (size_t)l0 * (size_t)g.S; qd.chunk0 = first + l0; qd.chunkRows = L;
        row_quantiles_launch(stream, cp, qd); launched();
      }
    }
  }
};

// uploads, per chunk the value kernel, the reduce and the fold, then the level kernels and the downloads — on `stream`, everything allocated here
// freed here (summary_run's discipline)
static void groups_run(hipStream_t stream, int P, const GroupsCall& c, int64_t& launches) {
  const ContrastCall& ar = c.arms;
  const bool two = c.nArms == 2;
  bool walks = true;
  SummaryCall r = two ? contrast_rows(ar, walks) : ar.rows;
  const ReadoutPlan plan = readout_plan(r, 0, two ? 8 : 4, false);
  const ChunkPlan cp = chunk_plan(r.nT, r.S, ar.scratchBytes, QT_SCRATCH_DEFAULT, 1, 64);
  CallBuffers buf(stream);
  const size_t nT = (size_t)r.nT, S = (size_t)r.S, Q = (size_t)ar.Q, L = (size_t)c.L;
  const int64_t slabsMax = (cp.C + GP_SLAB - 1) / GP_SLAB;
  // the levels that touch more than one slab, ascending
  std::vector<int32_t> edgeLevel;
  for (int64_t l = 0; l < c.L; ++l)
    if (c.levelStart[l + 1] > c.levelStart[l] && c.levelStart[l] / GP_SLAB != (c.levelStart[l + 1] - 1) / GP_SLAB) edgeLevel.push_back((int32_t)l);
  ContrastDev a{};
  if (two) contrast_upload(buf, a, ar, r, P, plan); else buf.upload_rows(a, r, P, plan.stageNodes);
  a.vals = buf.alloc<double>(nullptr, (size_t)cp.C * S);
  GroupsDev g{};
  g.vals = a.vals;
  g.level = buf.alloc(c.level, nT);
  if (c.rowWeights) g.w = buf.alloc(c.rowWeights, nT);
  g.lev = buf.alloc<double>(nullptr, L * S);
  g.edge = buf.alloc<double>(nullptr, (size_t)slabsMax * 2 * S);
  g.levelStart = buf.alloc(c.levelStart, L + 1);
  g.levelWeight = buf.alloc(c.levelWeight, L);
  g.edgeLevel = buf.alloc(edgeLevel.data(), edgeLevel.size());
  if (c.mean) g.mean = buf.alloc<double>(nullptr, L);
  if (c.m2) g.m2 = buf.alloc<double>(nullptr, L);
  if (c.pAbove) g.pAbove = buf.alloc<double>(nullptr, L);
  g.nT = r.nT; g.S = r.S; g.L = c.L; g.statistic = c.statistic; g.hasThreshold = c.hasThreshold; g.threshold = c.threshold;
  LevelsSummary sum;          // its sort alone: the levels here have tables, a statistic and a threshold of their own
  sum.prepare(buf, cp, r.S, ar.probs, ar.Q, 0);
  double* quantiles = Q ? buf.alloc<double>(nullptr, Q * L) : nullptr;
  arm_values_prepare(plan, two);
  LaunchCount launched{launches};
  size_t e0 = 0, e1 = 0;          // edgeLevel[e0 .. e1): the levels with rows in the chunk
  for (int64_t ch = 0; ch < cp.chunks; ++ch) {
    a.chunk0 = ch * cp.C; a.chunkRows = std::min<int64_t>(cp.C, r.nT - a.chunk0);
    g.chunk0 = a.chunk0; g.chunkRows = a.chunkRows;
    arm_values_launch(stream, plan, chunk_grid(a), a, two); launched();
    const int slabs = (int)((a.chunkRows + GP_SLAB - 1) / GP_SLAB);
    hipLaunchKernelGGL(k_level_reduce, dim3(slabs, (unsigned)((r.S + GP_BLOCK - 1) / GP_BLOCK)), dim3(GP_BLOCK), 0, stream, g); launched();
    const int64_t end = a.chunk0 + a.chunkRows;
    while (e0 < edgeLevel.size() && c.levelStart[edgeLevel[e0] + 1] <= a.chunk0) ++e0;
    e1 = std::max(e1, e0);
    while (e1 < edgeLevel.size() && c.levelStart[edgeLevel[e1]] < end) ++e1;
    if (e1 > e0) {
      const int64_t n = (int64_t)(e1 - e0) * r.S;
      hipLaunchKernelGGL(k_level_fold, dim3((unsigned)std::min<int64_t>(GRID_MAX, (n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, g, (int64_t)e0, (int64_t)(e1 - e0)); launched();
    }
  }
  hipLaunchKernelGGL(k_level_rows, dim3((unsigned)std::min<int64_t>(GRID_MAX, (c.L + BLOCK / 64 - 1) / (BLOCK / 64))), dim3(BLOCK), 0, stream, g); launched();
  if (Q) sum.run(stream, launched, g.lev, c.L, 0, nullptr, nullptr, quantiles, c.L);
  if (c.mean) HIP_OK(hipMemcpyAsync(c.mean, g.mean, L * 8, hipMemcpyDeviceToHost, stream));
  if (c.m2) HIP_OK(hipMemcpyAsync(c.m2, g.m2, L * 8, hipMemcpyDeviceToHost, stream));
  if (c.pAbove) HIP_OK(hipMemcpyAsync(c.pAbove, g.pAbove, L * 8, hipMemcpyDeviceToHost, stream));
  if (Q) HIP_OK(hipMemcpyAsync(c.quantiles, quantiles, Q * L * 8, hipMemcpyDeviceToHost, stream));
  if (c.draws) HIP_OK(hipMemcpyAsync(c.draws, g.lev, L * S * 8, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  r.info[0] = !walks ? 0 : plan.staged ? 1 : 2; r.info[1] = cp.C; r.info[2] = cp.chunks; r.info[3] = launched.mine;
  r.info[4] = buf.bytes; r.info[5] = r.S; r.info[6] = (int64_t)edgeLevel.size(); r.info[7] = c.nanLevels;
}
