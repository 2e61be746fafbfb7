// The spread of the rows' values ACROSS THE ROWS within one pooled draw, summarised over the draws (s4b_predict_spread; DESIGN.md 5.14): for rows
// i < n with weights w_i >= 0 and ascending thresholds t_0 < ... < t_{T-1}, T <= SP_THRESHOLDS_MAX, per pooled draw k
//     mean_k = sum_i w_i x(i,k) / W,   sd_k = sqrt(M2_k / W),   M2_k = sum_i w_i (x(i,k) - mean_k)^2,   min_k, max_k over the rows with w_i > 0,
//     share_above[j] = (sum of w_i over x(i,k) > t_j) / W,   part_above[j] = (sum of w_i x(i,k) over x(i,k) > t_j) / W,
//     x = k_predict_values' v (one arm) or k_contrast_values' d (two arms),
// the matrix D [(4 + 2 T) x S] of those statistics, and per statistic the mean, m2 and type-7 quantiles over the draws.
// Included by dev_hip.hip inside namespace s4b, after readout_projection.inc: the value kernels, the chunked scratch, the LDS sort, the call scaffold
// and the summary over the draws (k_level_rows, k_row_quantiles, unchanged) are dev_readout.inc's, dev_quantile.inc's, dev_contrast.inc's and
// dev_groups.inc's.  New here is the per-draw reduction that is not linear in the rows: a shifted second moment, the extremes and a weighted histogram
// over the thresholds.
//
// THE ORDER OF THE ADDITIONS (include/stan4bart_amd.h states it, tests/spread_cases.py models it): slabs are the GLOBAL blocks of SP_SLAB rows — a
// chunk starts on a multiple of SP_SLAB, so a slab never depends on the chunking.
//   Moments.  With c = the value of the slab's first row, W_s = fold of w_i, s1 = fold of w_i (x - c), s2 = fold of w_i (x - c)^2, left folds in row
//   order from +0 (a term and its addition may contract to one fused multiply-add); the slab's partial is (W_s, c + s1 / W_s, max(0, s2 - s1^2 / W_s)).
//   The partials combine over the slabs in ascending order by the pairwise update of Chan, Golub and LeVeque: delta = mean_b - mean_a,
//   W = W_a + W_b, mean = mean_a + delta W_b / W, M2 = M2_a + M2_b + delta^2 W_a W_b / W; a partial with W_s = 0 is skipped, the first partial with
//   W_s > 0 is taken as it is.
//   Bins.  bin(x) = #{j : x > t_j}; per slab and bin cw[b] = fold of w_i, cs[b] = fold of w_i x in row order from +0; over the slabs they are added in
//   ascending order; after the last chunk above_w[j] = sum_{b > j} cw[b] is added from b = T downward, above_s likewise.
//   Extremes are order-free.
// Per chunk of C rows (chunk_plan, in whole slabs of SP_SLAB rows):
//   k_predict_values<STAGED> / k_contrast_values<STAGED>   unchanged: the chunk's values row-major in the scratch.
//   k_spread_reduce<BINS, SEARCH>   one workgroup (a wave) per slab and block of SP_BLOCK draws, a draw per lane: vals[r S + k] is read coalesced
//                       across the wave, once; w[r] is a scalar load; the loads of SP_AHEAD = 8 rows are issued together (k_proj_reduce's shape).
//                       s1, s2, min, max and c stay in registers.  The bin of a lane's value differs from lane to lane, so cw and cs live in LDS,
//                       laid out [bin][lane]: lane l reads and writes only column l, the 64 lanes of one access touch 64 consecutive doubles (no
//                       bank conflict), and a lane's accesses stay in program order, so the kernel needs no barrier.  (T + 1) KiB of dynamic LDS,
//                       65 KiB at T = 64, set through hipFuncSetAttribute; BINS false (T = 0): no LDS at all.  The thresholds are the same for every
//                       lane: SEARCH false counts the compares x > t_j, t_j a scalar load shared by the 8 rows in flight; SEARCH true stages the
//                       thresholds in LDS behind the tables and finds the bin in ceil(log2(T + 1)) steps, each an LDS read at the lane's own index.
//                       Both give the same bin.  The slab's partials are stored coalesced: part[slab][5 + 2 (T + 1)][S] — W_s, mean_s, M2_s, min,
//                       max, cw[0 .. T], cs[0 .. T].
//   k_spread_fold       the running totals plus this chunk's partials in slab order: a thread per draw for the moments and the extremes, a thread per
//                       (bin, draw) for the bin sums.  The totals start at W = 0 and +0, so the first partial is taken as it is.
// After the last chunk:
//   k_spread_finish     a thread per draw: the suffix sums and the divisions by W (the host's sum of the weights in row order) into D.
//   k_level_rows, k_row_quantiles   unchanged, over D as 4 + 2 T levels of unit weight, statistic 0.  D holds no NaN: W > 0 is required.
// No floating-point atomics, no data-dependent order.  Device memory beyond the value kernel's: the weights, the thresholds, the partials
// 8 ceil(C / SP_SLAB) (5 + 2 (T + 1)) S, the totals 8 (5 + 2 (T + 1)) S, D and the summaries: nothing grows with n x S beyond the chunk.
constexpr int SP_SLAB = 128;                     // rows per slab: the unit of the fold, part of the interface (S4B_SPREAD_SLAB)
constexpr int SP_BLOCK = 64;                     // threads per workgroup of k_spread_reduce: one wave, a draw per lane
constexpr int SP_THRESHOLDS_MAX = 64;            // S4B_SPREAD_THRESHOLDS_MAX
constexpr int SP_AHEAD = 8;                      // rows of a slab whose loads k_spread_reduce keeps in flight together
constexpr int SP_MOMENTS = 5;                    // W_s, mean_s, M2_s, min, max: the rows of a partial in front of the bins
constexpr int SP_SEARCH_MIN = 32;                // thresholds from which the automatic choice searches instead of counting compares: where the two cross (DESIGN.md 5.14)

struct SpreadDev {
  const double* vals; const double* w;           // the chunk's values vals[r S + k]; [nT] or NULL (every weight 1)
  const double* thr;                             // [T] ascending
  double* part; double* tot;                     // [slabs of a chunk][5 + 2 (T + 1)][S], [5 + 2 (T + 1)][S]
  double* out;                                   // D [(4 + 2 T) x S]
  int64_t S, row0, rows;                         // the chunk's first row among all rows (a multiple of SP_SLAB) and its rows
  int T; double W;
};

// bin(x) = #{j : x > t_j} of the N values a lane holds, added onto bin[] (the caller's 0): SEARCH false counts the compares against thr[0 .. T), a
// scalar load per threshold shared by the N values; SEARCH true walks the thresholds staged in LDS at `tl` in ceil(log2(T + 1)) steps from `top`, the
// largest power of two <= T.  Both give the same bin.  (k_spread_reduce's, and readout_check.inc's k_check_reduce's.)
template <bool SEARCH, int N>
__device__ __forceinline__ void sp_bins(const double (&xs)[N], int (&bin)[N], int T, int top, const double* thr, const double* tl) {
  if (SEARCH) {
    for (int step = top; step; step >>= 1) {
#pragma unroll
      for (int u = 0; u < N; ++u) {
        const int q = bin[u] + step;
        if (q <= T && xs[u] > tl[q - 1]) bin[u] = q;
      }
    }
  } else {
    for (int j = 0; j < T; ++j) {
      const double t = thr[j];
#pragma unroll
      for (int u = 0; u < N; ++u) bin[u] += xs[u] > t ? 1 : 0;
    }
  }
}

template <bool BINS, bool SEARCH>
__global__ __launch_bounds__(SP_BLOCK) void k_spread_reduce(SpreadDev a) {
  extern __shared__ __attribute__((aligned(16))) double sp_lds[];                  // cw [T + 1][64], cs [T + 1][64], then (SEARCH) the thresholds [T]
  const int lane = threadIdx.x, T = a.T;
  const int64_t S = a.S, k = (int64_t)blockIdx.y * SP_BLOCK + lane;
  const bool mine = k < S;
  const int64_t r0 = (int64_t)blockIdx.x * SP_SLAB, g0 = a.row0 + r0;              // the slab's first row inside the chunk and among all rows
  const int rows = (int)min((int64_t)SP_SLAB, a.rows - r0);
  const double* __restrict__ w = a.w ? a.w + g0 : nullptr;                         // (the same for every lane: scalar loads)
  const double* __restrict__ thr = a.thr;
  const double* __restrict__ v = a.vals + (size_t)r0 * (size_t)S + (size_t)(mine ? k : S - 1);
  double* cw = sp_lds + lane;                                                      // cw[b * 64]: this lane's column
  double* cs = cw + (size_t)(T + 1) * SP_BLOCK;
  const double* tl = sp_lds + (size_t)2 * (T + 1) * SP_BLOCK;
  int top = 1;                                                                     // the largest power of two <= T
  if (BINS) {
    for (int b = 0; b <= T; ++b) { cw[b * SP_BLOCK] = 0.0; cs[b * SP_BLOCK] = 0.0; }
    if (SEARCH) {
      for (int j = lane; j < T; j += SP_BLOCK) sp_lds[(size_t)2 * (T + 1) * SP_BLOCK + j] = thr[j];
      __syncthreads();                                                             // (one wave: the thresholds other lanes staged)
      while (top * 2 <= T) top *= 2;
    }
  }
  const double c = v[0];
  double Ws = 0.0, s1 = 0.0, s2 = 0.0;
  double mn = __longlong_as_double(0x7ff0000000000000ll), mx = -mn;
  for (int r = 0; r < rows; r += SP_AHEAD) {
    double xs[SP_AHEAD], ws[SP_AHEAD];
    int bin[SP_AHEAD];
#pragma unroll
    for (int u = 0; u < SP_AHEAD; ++u) {                                           // the loads of SP_AHEAD rows in flight together (past the slab's end: its last row again)
      const int q = min(r + u, rows - 1);
      xs[u] = v[(size_t)q * (size_t)S];
      ws[u] = w ? w[q] : 1.0;
      bin[u] = 0;
    }
    if (BINS) sp_bins<SEARCH, SP_AHEAD>(xs, bin, T, top, thr, tl);
#pragma unroll
    for (int u = 0; u < SP_AHEAD; ++u) {
      if (r + u < rows) {                                                          // (the same for every lane)
        const double x = xs[u], wi = ws[u], d = x - c;
        const double wd = w ? wi * d : d, wx = w ? wi * x : x;
        Ws += wi; s1 += wd; s2 += wd * d;
        if (wi > 0.0) { mn = fmin(mn, x); mx = fmax(mx, x); }                      // (the same for every lane)
        if (BINS) {
          const int b = bin[u] * SP_BLOCK;
          cw[b] += wi; cs[b] += wx;
        }
      }
    }
  }
  if (!mine) return;
  const int64_t R = SP_MOMENTS + 2 * (T + 1);
  double* out = a.part + (size_t)blockIdx.x * (size_t)R * (size_t)S + (size_t)k;
  const bool any = Ws > 0.0;
  out[0] = Ws;
  out[(size_t)S] = any ? c + s1 / Ws : 0.0;
  out[(size_t)2 * (size_t)S] = any ? fmax(0.0, s2 - s1 * s1 / Ws) : 0.0;
  out[(size_t)3 * (size_t)S] = mn;
  out[(size_t)4 * (size_t)S] = mx;
  if (BINS)
    for (int b = 0; b <= T; ++b) {
      out[(size_t)(SP_MOMENTS + b) * (size_t)S] = cw[b * SP_BLOCK];
      out[(size_t)(SP_MOMENTS + T + 1 + b) * (size_t)S] = cs[b * SP_BLOCK];
    }
}

__global__ __launch_bounds__(BLOCK) void k_spread_fold(SpreadDev a) {
  const int64_t S = a.S, R = SP_MOMENTS + 2 * (a.T + 1), slabs = (a.rows + SP_SLAB - 1) / SP_SLAB;
  const int64_t m = S + (a.T > 0 ? 2 * (int64_t)(a.T + 1) * S : 0);
  for (int64_t x = (int64_t)blockIdx.x * BLOCK + threadIdx.x; x < m; x += (int64_t)gridDim.x * BLOCK) {
    if (x < S) {                                                                   // the moments and the extremes of draw x
      double* t = a.tot + (size_t)x;
      double Wa = t[0], mean = t[(size_t)S], M2 = t[(size_t)2 * (size_t)S], mn = t[(size_t)3 * (size_t)S], mx = t[(size_t)4 * (size_t)S];
      for (int64_t s0 = 0; s0 < slabs; s0 += SP_AHEAD) {
        double pw[SP_AHEAD], pm[SP_AHEAD], pq[SP_AHEAD], lo[SP_AHEAD], hi[SP_AHEAD];
#pragma unroll
        for (int u = 0; u < SP_AHEAD; ++u) {                                       // the loads of SP_AHEAD slabs in flight together: the update below is one serial chain
          const double* p = a.part + (size_t)min(s0 + u, slabs - 1) * (size_t)R * (size_t)S + (size_t)x;
          pw[u] = p[0]; pm[u] = p[(size_t)S]; pq[u] = p[(size_t)2 * (size_t)S]; lo[u] = p[(size_t)3 * (size_t)S]; hi[u] = p[(size_t)4 * (size_t)S];
        }
#pragma unroll
        for (int u = 0; u < SP_AHEAD; ++u) {
          const double Wb = pw[u];
          if (s0 + u >= slabs || !(Wb > 0.0)) continue;                            // (past the chunk's end;) a slab without weight
          mn = fmin(mn, lo[u]); mx = fmax(mx, hi[u]);
          if (!(Wa > 0.0)) { Wa = Wb; mean = pm[u]; M2 = pq[u]; continue; }        // the first partial with weight: as it is
          const double delta = pm[u] - mean, W = Wa + Wb;
          mean = mean + delta * Wb / W;
          M2 = M2 + pq[u] + delta * delta * Wa * Wb / W;
          Wa = W;
        }
      }
      t[0] = Wa; t[(size_t)S] = mean; t[(size_t)2 * (size_t)S] = M2; t[(size_t)3 * (size_t)S] = mn; t[(size_t)4 * (size_t)S] = mx;
    } else {                                                                       // a bin sum: rows SP_MOMENTS .. of the partials, contiguous
      const size_t e = (size_t)SP_MOMENTS * (size_t)S + (size_t)(x - S);
      double acc = a.tot[e];
#pragma unroll 8
      for (int64_t sl = 0; sl < slabs; ++sl) acc += a.part[(size_t)sl * (size_t)R * (size_t)S + e];
      a.tot[e] = acc;
    }
  }
}

__global__ __launch_bounds__(BLOCK) void k_spread_finish(SpreadDev a) {
  const int64_t S = a.S;
  const int T = a.T;
  for (int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x; k < S; k += (int64_t)gridDim.x * BLOCK) {
    const double* t = a.tot + (size_t)k;
    double* o = a.out + (size_t)k;
    o[0] = t[(size_t)S];
    o[(size_t)S] = sqrt(t[(size_t)2 * (size_t)S] / a.W);
    o[(size_t)2 * (size_t)S] = t[(size_t)3 * (size_t)S];
    o[(size_t)3 * (size_t)S] = t[(size_t)4 * (size_t)S];
    double aw = 0.0, as = 0.0;
    for (int b = T; b >= 1; --b) {                                                 // above[j] = sum_{b > j}: from the top bin downward
      aw += t[(size_t)(SP_MOMENTS + b) * (size_t)S];
      as += t[(size_t)(SP_MOMENTS + T + 1 + b) * (size_t)S];
      o[(size_t)(4 + b - 1) * (size_t)S] = aw / a.W;
      o[(size_t)(4 + T + b - 1) * (size_t)S] = as / a.W;
    }
  }
}

// uploads, per chunk the value kernel, the reduce and the fold, then the finish, the summary kernels and the downloads — on `stream`, everything
// allocated here freed here (summary_run's discipline)
static void spread_run(hipStream_t stream, int P, const SpreadCall& c, int64_t& launches) {
  const ContrastCall& ar = c.arms;
  const bool two = c.nArms == 2;
  bool walks = true;
  SummaryCall r = two ? contrast_rows(ar, walks) : ar.rows;
  const ReadoutPlan plan = readout_plan(r, 0, two ? 8 : 4, false);
  const ChunkPlan cp = chunk_plan(r.nT, r.S, ar.scratchBytes, QT_SCRATCH_DEFAULT, 1, SP_SLAB);          // whole slabs
  CallBuffers buf(stream);
  const size_t nT = (size_t)r.nT, S = (size_t)r.S, Q = (size_t)ar.Q, T = (size_t)c.T, L = 4 + 2 * T, R = SP_MOMENTS + 2 * (T + 1);
  const int64_t C = cp.C, slabsMax = (C + SP_SLAB - 1) / SP_SLAB;
  const bool search = c.T > 0 && (c.binIndex == 2 || (c.binIndex == 0 && c.T >= SP_SEARCH_MIN));
  const size_t binLds = T ? (2 * (T + 1) * SP_BLOCK + (search ? T : 0)) * 8 : 0;
  ContrastDev a{};
  if (two) contrast_upload(buf, a, ar, r, P, plan); else buf.upload_rows(a, r, P, plan.stageNodes);
  a.vals = buf.alloc<double>(nullptr, (size_t)C * S);
  SpreadDev p{};
  p.vals = a.vals;
  if (c.rowWeights) p.w = buf.alloc(c.rowWeights, nT);
  if (T) p.thr = buf.alloc(c.thresholds, T);
  p.part = buf.alloc<double>(nullptr, (size_t)slabsMax * R * S);
  // the totals: W = 0 (no partial yet), +0 in every sum, the extremes at +-inf
  std::vector<double> init(R * S, 0.0);
  std::fill(init.begin() + 3 * S, init.begin() + 4 * S, std::numeric_limits<double>::infinity());
  std::fill(init.begin() + 4 * S, init.begin() + 5 * S, -std::numeric_limits<double>::infinity());
  p.tot = buf.alloc(init.data(), R * S);
  p.out = buf.alloc<double>(nullptr, L * S);
  p.S = r.S; p.T = c.T; p.W = c.W;
  LevelsSummary sum;          // D's 4 + 2 T rows as levels of unit weight
  sum.prepare(buf, cp, r.S, ar.probs, ar.Q, (int64_t)L);
  double* mean = c.mean ? buf.alloc<double>(nullptr, L) : nullptr;
  double* m2 = c.m2 ? buf.alloc<double>(nullptr, L) : nullptr;
  double* quantiles = Q ? buf.alloc<double>(nullptr, Q * L) : nullptr;
  arm_values_prepare(plan, two);
  if (T) {
    if (search) HIP_OK(hipFuncSetAttribute((const void*)k_spread_reduce<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)binLds));
    else HIP_OK(hipFuncSetAttribute((const void*)k_spread_reduce<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)binLds));
  }
  LaunchCount launched{launches};
  for (int64_t ch = 0; ch < cp.chunks; ++ch) {
    a.chunk0 = ch * C; a.chunkRows = std::min<int64_t>(C, r.nT - a.chunk0);
    arm_values_launch(stream, plan, chunk_grid(a), a, two); launched();
    p.row0 = a.chunk0; p.rows = a.chunkRows;
    const dim3 grid((unsigned)((p.rows + SP_SLAB - 1) / SP_SLAB), (unsigned)((r.S + SP_BLOCK - 1) / SP_BLOCK));
    if (!T) hipLaunchKernelGGL((k_spread_reduce<false, false>), grid, dim3(SP_BLOCK), 0, stream, p);
    else if (search) hipLaunchKernelGGL((k_spread_reduce<true, true>), grid, dim3(SP_BLOCK), binLds, stream, p);
    else hipLaunchKernelGGL((k_spread_reduce<true, false>), grid, dim3(SP_BLOCK), binLds, stream, p);
    launched();
    const int64_t m = r.S + (T ? 2 * (int64_t)(T + 1) * r.S : 0);
    hipLaunchKernelGGL(k_spread_fold, dim3((unsigned)std::min<int64_t>(GRID_MAX, (m + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, p); launched();
  }
  hipLaunchKernelGGL(k_spread_finish, dim3((unsigned)std::min<int64_t>(GRID_MAX, (r.S + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, p); launched();
  sum.run(stream, launched, p.out, (int64_t)L, 0, mean, m2, quantiles, (int64_t)L);
  if (mean) HIP_OK(hipMemcpyAsync(c.mean, mean, L * 8, hipMemcpyDeviceToHost, stream));
  if (m2) HIP_OK(hipMemcpyAsync(c.m2, m2, L * 8, hipMemcpyDeviceToHost, stream));
  if (Q) HIP_OK(hipMemcpyAsync(c.quantiles, quantiles, Q * L * 8, hipMemcpyDeviceToHost, stream));
  if (c.draws) HIP_OK(hipMemcpyAsync(c.draws, p.out, L * S * 8, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  r.info[0] = !walks ? 0 : plan.staged ? 1 : 2; r.info[1] = C; r.info[2] = cp.chunks; r.info[3] = launched.mine;
  r.info[4] = buf.bytes; r.info[5] = r.S; r.info[6] = c.T; r.info[7] = c.zeroSlabs;
}
