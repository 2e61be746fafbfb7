// Posterior predictive checks (s4b_predict_check; DESIGN.md 5.15): statistics of the REPLICATE y_rep ACROSS THE ROWS within one pooled draw, each to be
// held against the same statistic of the observed y, summarised over the draws.  For rows i < n with responses y_i, weights w_i >= 0 and ascending
// thresholds t_0 < ... < t_{T-1}, T <= SP_THRESHOLDS_MAX, per pooled draw k, with x(i,k) = y_rep(i,k):
//     link 0:  x = z + sd e,  sd = sigma[k] row_scale[i],  e = philox_normal(key, i, k)      (the bits k_ppd_rows sorts under the same key)
//     link 1:  x = 1 where u <= Phi(z), else 0,  u = philox_uniform(key, i, k),  Phi = readout_phi
//     mean_k = sum_i w_i x / W,   sd_k = sqrt(M2_k / W),   m3_k = M3_k / W   (M2, M3 the weighted central sums),   min_k, max_k over the rows with w_i > 0,
//     share_above[j] = (sum of w_i over x > t_j) / W,
//     link 0:  disc_rep = sum_i w_i e^2 / W,   disc_obs = sum_i w_i ((y_i - z) / sd)^2 / W                     (chi^2 of Gelman, Meng and Stern)
//     link 1:  disc = -2 sum_i w_i log Phi(+-z) / W, the sign from y_rep (disc_rep) or from y_i (disc_obs)     (the deviance)
// the matrix D [(7 + T) x S]: mean, sd, m3, min, max, share_above[0 .. T), disc_rep, disc_obs, and per row of D the mean, m2 and type-7 quantiles over
// the draws.  observed[5 + T]: mean, sd, m3, min, max, share_above of y itself, formed on the host by the routines below that the kernels run too.
// z(i,k) is what k_predict_values writes with link 0, as k_ppd_rows takes it; i is the row OF THE CALL and k the pooled draw, so the replicate does
// not depend on chunking, route or sampler kind.  The replicate is formed in registers and never stored.
// Included by dev_hip.hip inside namespace s4b, after readout_spread.inc: the slab, the lane layout, the bin routine (sp_bins) and the constants
// SP_* are readout_spread.inc's; the value kernel, the chunked scratch and the summary over the draws (k_level_rows, k_row_quantiles, unchanged)
// are dev_readout.inc's, dev_quantile.inc's and dev_groups.inc's; the generator is philox.hpp's.
//
// THE ORDER OF THE ADDITIONS (include/stan4bart_amd.h states it, tests/check_cases.py models it): slabs are the GLOBAL blocks of SP_SLAB rows.
//   Moments.  With c = the replicate of the slab's first row and d_i = x_i - c: W_s = fold of w_i, s1 = fold of w_i d_i, s2 = fold of (w_i d_i) d_i,
//   s3 = fold of ((w_i d_i) d_i) d_i, left folds in row order from +0 (a term and its addition may contract to one fused multiply-add): ck_add.  With
//   d = s1 / W_s the slab's partial is (W_s, c + d, max(0, s2 - d s1), (s3 - 3 d s2) + 2 d^2 s1): ck_partial.  The partials combine over the slabs in
//   ascending order by the pairwise update (ck_combine): delta = mean_b - mean_a, W = W_a + W_b,
//       M3 = M3_a + M3_b + delta^3 W_a W_b (W_a - W_b) / W^2 + 3 delta (W_a M2_b - W_b M2_a) / W           (Pebay)
//       M2 = M2_a + M2_b + delta^2 W_a W_b / W,   mean = mean_a + delta W_b / W                            (Chan, Golub and LeVeque; 5.14's)
//   a partial with W_s = 0 is skipped, the first partial with W_s > 0 is taken as it is.
//   Bins.  bin(x) = #{j : x > t_j}; per slab and bin cw[b] = fold of w_i in row order from +0; over the slabs added in ascending order; after the
//   last chunk above_w[j] = sum_{b > j} cw[b] from b = T downward.  Only the weights are counted.
//   Discrepancies.  Per slab the left folds of w_i (e e), w_i (r r) with r = (y_i - z) / sd (link 0) or of w_i log Phi(+-z) (link 1) in row order
//   from +0, a row with w_i = 0 adding no term (under link 1 its log Phi may be -inf: 0 x -inf is not formed); over the slabs added in ascending
//   order; D holds total / W (link 0) and (-2 total) / W (link 1).
//   Extremes are order-free.
// Per chunk of C rows (chunk_plan, in whole slabs of SP_SLAB rows):
//   k_predict_values<STAGED>   unchanged, link 0: the chunk's z row-major in the scratch.
//   k_check_reduce<LINK, BINS, SEARCH> k_spread_reduce's shape: one wave per slab and block of SP_BLOCK draws, a draw per lane; the loads of CK_AHEAD rows of
//                       z are issued together; w, y and row_scale of a row are wave-uniform loads; sigma[k] is loaded once per lane.  Per row the
//                       Philox block, Box-Muller or the uniform and the replicate; s1, s2, s3, c, the extremes and the two discrepancy sums stay in
//                       registers.  The weight histogram lives in dynamic LDS, [bin][lane], (T + 1) x 512 bytes (33 KiB at T = 64): lane l touches
//                       only column l, so there is no bank conflict and no barrier (5.14).  SEARCH chooses sp_bins' route (the same bin), a template parameter as in k_spread_reduce.  The
//                       slab's partials are stored coalesced: part[slab][R][S], R = CK_MOMENTS + (T + 1 with thresholds) — W_s, mean_s, M2_s, M3_s,
//                       min, max, the two discrepancy sums, cw[0 .. T].
//   k_check_fold        the running totals plus this chunk's partials in slab order: a thread per draw for the moments, the extremes and the
//                       discrepancy sums (the loads of CK_SLABS_AHEAD slabs issued together), a thread per (bin, draw) for the bin sums.
// After the last chunk:
//   k_check_finish      a thread per draw: the suffix sums and the divisions by W (the host's sum of the weights in row order) into D.
//   k_level_rows, k_row_quantiles   unchanged, over D as 7 + T levels of unit weight, statistic 0.  D holds no NaN: W > 0 is required.
// No floating-point atomics, no data-dependent order.  Device memory beyond the value kernel's: y, the weights, sigma,
// row_scale, the thresholds, the partials 8 ceil(C / SP_SLAB) R S, the totals 8 R S, D and the summaries: nothing grows with n x S beyond the chunk.
constexpr int CK_AHEAD = 4;                      // rows of a slab whose loads k_check_reduce keeps in flight together (with 8 the Philox rounds and Box-Muller beside them take 143 - 230 VGPRs, 2 - 3 waves per SIMD, and spill scalar registers; with 4 118 - 134, 3 - 4, no spill: DESIGN.md 5.15)
constexpr int CK_SLABS_AHEAD = 8;                // slabs whose partials k_check_fold keeps in flight together
constexpr int CK_MOMENTS = 8;                    // W_s, mean_s, M2_s, M3_s, min, max, disc_rep, disc_obs: the rows of a partial in front of the bins
constexpr int CK_STATS = 7;                      // rows of D beside the shares: mean, sd, m3, min, max, disc_rep, disc_obs

// ---- the stated order, once: the kernels and the host's statistics of y run these three
// one row onto the slab's shifted sums
__host__ __device__ __forceinline__ void ck_add(double x, double w, double c, double& Ws, double& s1, double& s2, double& s3) {
  const double d = x - c, wd = w * d, wdd = wd * d;
  Ws += w; s1 += wd; s2 += wdd; s3 += wdd * d;
}
// the slab's partial from its shifted sums (W_s > 0)
__host__ __device__ __forceinline__ void ck_partial(double Ws, double c, double s1, double s2, double s3, double& mean, double& M2, double& M3) {
  const double d = s1 / Ws;
  mean = c + d;
  M2 = fmax(0.0, s2 - d * s1);
  M3 = (s3 - 3.0 * d * s2) + 2.0 * d * d * s1;
}
// partial b (W_b > 0) onto the running totals a
__host__ __device__ __forceinline__ void ck_combine(double& Wa, double& mean, double& M2, double& M3, double Wb, double mb, double M2b, double M3b) {
  if (!(Wa > 0.0)) { Wa = Wb; mean = mb; M2 = M2b; M3 = M3b; return; }          // the first partial with weight: as it is
  const double delta = mb - mean, W = Wa + Wb;
  M3 = M3 + M3b + delta * delta * delta * Wa * Wb * (Wa - Wb) / (W * W) + 3.0 * delta * (Wa * M2b - Wb * M2) / W;
  M2 = M2 + M2b + delta * delta * Wa * Wb / W;
  mean = mean + delta * Wb / W;
  Wa = W;
}

struct CheckDev {
  const double* vals; const double* w;           // the chunk's z vals[r S + k]; [nT] or NULL (every weight 1)
  const double* y; const double* sigma; const double* rowScale;          // [nT]; [S] (link 0); [nT] or NULL (= 1)
  const double* thr;                             // [T] ascending
  double* part; double* tot;                     // [slabs of a chunk][R][S], [R][S]
  double* out;                                   // D [(7 + T) x S]
  int64_t S, row0, rows;                         // the chunk's first row among all rows (a multiple of SP_SLAB) and its rows
  int T, link; double W;
  uint32_t key0, key1;
};

template <int LINK, bool BINS, bool SEARCH>
__global__ __launch_bounds__(SP_BLOCK) void k_check_reduce(CheckDev a) {
  extern __shared__ __attribute__((aligned(16))) double ck_lds[];                  // cw [T + 1][64], then (SEARCH) the thresholds [T]
  const int lane = threadIdx.x, T = a.T;
  const int64_t S = a.S, k = (int64_t)blockIdx.y * SP_BLOCK + lane;
  const bool mine = k < S;
  const int64_t kk = mine ? k : S - 1;                                             // (a lane past the last draw forms the last draw's again and stores nothing)
  const int64_t r0 = (int64_t)blockIdx.x * SP_SLAB, g0 = a.row0 + r0;              // the slab's first row inside the chunk and among all rows
  const int rows = (int)min((int64_t)SP_SLAB, a.rows - r0);
  const double* __restrict__ w = a.w ? a.w + g0 : nullptr;                         // (the same for every lane: scalar loads)
  const double* __restrict__ y = a.y + g0;
  const double* __restrict__ rsc = (!LINK && a.rowScale) ? a.rowScale + g0 : nullptr;
  const double* __restrict__ thr = a.thr;
  const double* __restrict__ v = a.vals + (size_t)r0 * (size_t)S + (size_t)kk;
  const double sg = LINK ? 1.0 : a.sigma[kk];
  const uint32_t key0 = a.key0, key1 = a.key1, kd = (uint32_t)kk;
  double* cw = ck_lds + lane;                                                      // cw[b * 64]: this lane's column
  const double* tl = ck_lds + (size_t)(T + 1) * SP_BLOCK;
  int top = 1;                                                                     // the largest power of two <= T
  if (BINS) {
    for (int b = 0; b <= T; ++b) cw[b * SP_BLOCK] = 0.0;
    if (SEARCH) {
      for (int j = lane; j < T; j += SP_BLOCK) ck_lds[(size_t)(T + 1) * SP_BLOCK + j] = thr[j];
      __syncthreads();                                                             // (one wave: the thresholds other lanes staged)
      while (top * 2 <= T) top *= 2;
    }
  }
  double c = 0.0, Ws = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, dr = 0.0, dob = 0.0;
  double mn = __longlong_as_double(0x7ff0000000000000ll), mx = -mn;
  for (int r = 0; r < rows; r += CK_AHEAD) {
    double xs[CK_AHEAD];
    int bin[CK_AHEAD];
#pragma unroll
    for (int u = 0; u < CK_AHEAD; ++u)                                             // the loads of CK_AHEAD rows in flight together (past the slab's end: its last row again)
      xs[u] = v[(size_t)min(r + u, rows - 1) * (size_t)S];
#pragma unroll
    for (int u = 0; u < CK_AHEAD; ++u) {                                           // the replicate, in place of z
      const int q = min(r + u, rows - 1);
      const bool live = r + u < rows;                                              // (the same for every lane)
      const double z = xs[u], wi = w ? w[q] : 1.0, yi = y[q];
      const uint64_t row = (uint64_t)(g0 + q);
      if (LINK) {
        const double pz = readout_phi(z), lp = log(pz), lm = log(readout_phi(-z));
        const double x = philox_uniform(key0, key1, row, kd) <= pz ? 1.0 : 0.0;
        if (live && wi > 0.0) { dr += wi * (x > 0.0 ? lp : lm); dob += wi * (yi > 0.0 ? lp : lm); }          // (a row without weight adds nothing: 0 x -inf is no term)
        xs[u] = x;
      } else {
        const double sd = sg * (rsc ? rsc[q] : 1.0), e = philox_normal(key0, key1, row, kd), res = (yi - z) / sd;
        if (live && wi > 0.0) { dr += wi * (e * e); dob += wi * (res * res); }
        xs[u] = z + sd * e;
      }
      bin[u] = 0;
    }
    if (r == 0) c = xs[0];
    if (BINS) sp_bins<SEARCH, CK_AHEAD>(xs, bin, T, top, thr, tl);
#pragma unroll
    for (int u = 0; u < CK_AHEAD; ++u) {
      if (r + u < rows) {                                                          // (the same for every lane)
        const double x = xs[u], wi = w ? w[r + u] : 1.0;                           // (a scalar load again: not held across the bin search)
        ck_add(x, wi, c, Ws, s1, s2, s3);
        if (wi > 0.0) { mn = fmin(mn, x); mx = fmax(mx, x); }                      // (the same for every lane)
        if (BINS) cw[bin[u] * SP_BLOCK] += wi;
      }
    }
  }
  if (!mine) return;
  const int64_t R = CK_MOMENTS + (BINS ? T + 1 : 0);
  double* out = a.part + (size_t)blockIdx.x * (size_t)R * (size_t)S + (size_t)k;
  double mean = 0.0, M2 = 0.0, M3 = 0.0;
  if (Ws > 0.0) ck_partial(Ws, c, s1, s2, s3, mean, M2, M3);
  out[0] = Ws;
  out[(size_t)S] = mean;
  out[(size_t)2 * (size_t)S] = M2;
  out[(size_t)3 * (size_t)S] = M3;
  out[(size_t)4 * (size_t)S] = mn;
  out[(size_t)5 * (size_t)S] = mx;
  out[(size_t)6 * (size_t)S] = dr;
  out[(size_t)7 * (size_t)S] = dob;
  if (BINS)
    for (int b = 0; b <= T; ++b) out[(size_t)(CK_MOMENTS + b) * (size_t)S] = cw[b * SP_BLOCK];
}

__global__ __launch_bounds__(BLOCK) void k_check_fold(CheckDev a) {
  const int64_t S = a.S, R = CK_MOMENTS + (a.T > 0 ? a.T + 1 : 0), slabs = (a.rows + SP_SLAB - 1) / SP_SLAB;
  const int64_t m = S + (a.T > 0 ? (int64_t)(a.T + 1) * S : 0);
  for (int64_t x = (int64_t)blockIdx.x * BLOCK + threadIdx.x; x < m; x += (int64_t)gridDim.x * BLOCK) {
    if (x < S) {                                                                   // the moments, the extremes and the discrepancy sums of draw x
      double* t = a.tot + (size_t)x;
      double Wa = t[0], mean = t[(size_t)S], M2 = t[(size_t)2 * (size_t)S], M3 = t[(size_t)3 * (size_t)S];
      double mn = t[(size_t)4 * (size_t)S], mx = t[(size_t)5 * (size_t)S], dr = t[(size_t)6 * (size_t)S], dob = t[(size_t)7 * (size_t)S];
      for (int64_t s0 = 0; s0 < slabs; s0 += CK_SLABS_AHEAD) {
        double p[CK_SLABS_AHEAD][CK_MOMENTS];
#pragma unroll
        for (int u = 0; u < CK_SLABS_AHEAD; ++u) {                                       // the loads of CK_SLABS_AHEAD slabs in flight together: the update below is one serial chain
          const double* q = a.part + (size_t)min(s0 + u, slabs - 1) * (size_t)R * (size_t)S + (size_t)x;
#pragma unroll
          for (int j = 0; j < CK_MOMENTS; ++j) p[u][j] = q[(size_t)j * (size_t)S];
        }
#pragma unroll
        for (int u = 0; u < CK_SLABS_AHEAD; ++u) {
          if (s0 + u >= slabs) continue;                                           // past the chunk's end
          dr += p[u][6]; dob += p[u][7];
          if (!(p[u][0] > 0.0)) continue;                                          // a slab without weight
          mn = fmin(mn, p[u][4]); mx = fmax(mx, p[u][5]);
          ck_combine(Wa, mean, M2, M3, p[u][0], p[u][1], p[u][2], p[u][3]);
        }
      }
      t[0] = Wa; t[(size_t)S] = mean; t[(size_t)2 * (size_t)S] = M2; t[(size_t)3 * (size_t)S] = M3;
      t[(size_t)4 * (size_t)S] = mn; t[(size_t)5 * (size_t)S] = mx; t[(size_t)6 * (size_t)S] = dr; t[(size_t)7 * (size_t)S] = dob;
    } else {                                                                       // a bin sum: rows CK_MOMENTS .. of the partials, contiguous
      const size_t e = (size_t)CK_MOMENTS * (size_t)S + (size_t)(x - S);
      double acc = a.tot[e];
#pragma unroll 8
      for (int64_t sl = 0; sl < slabs; ++sl) acc += a.part[(size_t)sl * (size_t)R * (size_t)S + e];
      a.tot[e] = acc;
    }
  }
}

__global__ __launch_bounds__(BLOCK) void k_check_finish(CheckDev a) {
  const int64_t S = a.S;
  const int T = a.T;
  for (int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x; k < S; k += (int64_t)gridDim.x * BLOCK) {
    const double* t = a.tot + (size_t)k;
    double* o = a.out + (size_t)k;
    o[0] = t[(size_t)S];
    o[(size_t)S] = sqrt(t[(size_t)2 * (size_t)S] / a.W);
    o[(size_t)2 * (size_t)S] = t[(size_t)3 * (size_t)S] / a.W;
    o[(size_t)3 * (size_t)S] = t[(size_t)4 * (size_t)S];
    o[(size_t)4 * (size_t)S] = t[(size_t)5 * (size_t)S];
    double aw = 0.0;
    for (int b = T; b >= 1; --b) {                                                 // above[j] = sum_{b > j}: from the top bin downward
      aw += t[(size_t)(CK_MOMENTS + b) * (size_t)S];
      o[(size_t)(5 + b - 1) * (size_t)S] = aw / a.W;
    }
    const double dr = t[(size_t)6 * (size_t)S], dob = t[(size_t)7 * (size_t)S];
    o[(size_t)(5 + T) * (size_t)S] = (a.link ? -2.0 * dr : dr) / a.W;
    o[(size_t)(6 + T) * (size_t)S] = (a.link ? -2.0 * dob : dob) / a.W;
  }
}

// observed[5 + T]: mean, sd, m3, min, max and share_above of y itself, by the stated order with x = y (the shift of a slab is its first y)
static void check_observed(const double* y, const double* w, int64_t n, int T, const double* thr, double W, double* observed) {
  double Wa = 0.0, mean = 0.0, M2 = 0.0, M3 = 0.0;
  double mn = std::numeric_limits<double>::infinity(), mx = -mn;
  std::vector<double> cw((size_t)T + 1, 0.0), pw((size_t)T + 1);
  for (int64_t r0 = 0; r0 < n; r0 += SP_SLAB) {
    const int64_t r1 = std::min<int64_t>(n, r0 + SP_SLAB);
    const double c = y[r0];
    double Ws = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    std::fill(pw.begin(), pw.end(), 0.0);
    for (int64_t i = r0; i < r1; ++i) {
      const double x = y[i], wi = w ? w[i] : 1.0;
      ck_add(x, wi, c, Ws, s1, s2, s3);
      if (wi > 0.0) { mn = std::fmin(mn, x); mx = std::fmax(mx, x); }
      int b = 0;
      for (int j = 0; j < T; ++j) b += x > thr[j] ? 1 : 0;
      pw[(size_t)b] += wi;
    }
    for (int b = 0; b <= T; ++b) cw[(size_t)b] += pw[(size_t)b];
    if (!(Ws > 0.0)) continue;
    double ms, M2s, M3s;
    ck_partial(Ws, c, s1, s2, s3, ms, M2s, M3s);
    ck_combine(Wa, mean, M2, M3, Ws, ms, M2s, M3s);
  }
  observed[0] = mean; observed[1] = std::sqrt(M2 / W); observed[2] = M3 / W; observed[3] = mn; observed[4] = mx;
  double aw = 0.0;
  for (int b = T; b >= 1; --b) { aw += cw[(size_t)b]; observed[5 + b - 1] = aw / W; }
}

// uploads, per chunk the value kernel, the reduce and the fold, then the finish, the summary kernels and the downloads — on `stream`, everything
// allocated here freed here (summary_run's discipline)
static void check_run(hipStream_t stream, int P, const CheckCall& c, int64_t& launches) {
  SummaryCall r = c.rows;
  const int link = r.link;
  r.link = 0;                                                     // k_predict_values writes z, whatever the response
  const ReadoutPlan plan = readout_plan(r, 0, 4, false);
  const ChunkPlan cp = chunk_plan(r.nT, r.S, c.scratchBytes, QT_SCRATCH_DEFAULT, 1, SP_SLAB);          // whole slabs
  CallBuffers buf(stream);
  const size_t nT = (size_t)r.nT, S = (size_t)r.S, Q = (size_t)c.Q, T = (size_t)c.T, L = CK_STATS + T, R = CK_MOMENTS + (T ? T + 1 : 0);
  const int64_t C = cp.C, slabsMax = (C + SP_SLAB - 1) / SP_SLAB;
  const bool search = c.T > 0 && (c.binIndex == 2 || (c.binIndex == 0 && c.T >= SP_SEARCH_MIN));
  const size_t binLds = T ? ((T + 1) * SP_BLOCK + (search ? T : 0)) * 8 : 0;
  if (c.observed) check_observed(c.y, c.rowWeights, r.nT, c.T, c.thresholds, c.W, c.observed);
  QuantileDev a{};
  buf.upload_rows(a, r, P, plan.stageNodes);
  a.vals = buf.alloc<double>(nullptr, (size_t)C * S);
  CheckDev p{};
  p.vals = a.vals;
  p.y = buf.alloc(c.y, nT);
  if (c.rowWeights) p.w = buf.alloc(c.rowWeights, nT);
  if (!link) { p.sigma = buf.alloc(c.sigma, S); if (c.rowScale) p.rowScale = buf.alloc(c.rowScale, nT); }
  if (T) p.thr = buf.alloc(c.thresholds, T);
  p.part = buf.alloc<double>(nullptr, (size_t)slabsMax * R * S);
  // the totals: W = 0 (no partial yet), +0 in every sum, the extremes at +-inf
  std::vector<double> init(R * S, 0.0);
  std::fill(init.begin() + 4 * S, init.begin() + 5 * S, std::numeric_limits<double>::infinity());
  std::fill(init.begin() + 5 * S, init.begin() + 6 * S, -std::numeric_limits<double>::infinity());
  p.tot = buf.alloc(init.data(), R * S);
  p.out = buf.alloc<double>(nullptr, L * S);
  p.S = r.S; p.T = c.T; p.link = link; p.W = c.W;
  p.key0 = (uint32_t)c.noiseKey; p.key1 = (uint32_t)(c.noiseKey >> 32);
  LevelsSummary sum;          // D's 7 + T rows as levels of unit weight
  sum.prepare(buf, cp, r.S, c.probs, c.Q, (int64_t)L);
  double* mean = c.mean ? buf.alloc<double>(nullptr, L) : nullptr;
  double* m2 = c.m2 ? buf.alloc<double>(nullptr, L) : nullptr;
  double* quantiles = Q ? buf.alloc<double>(nullptr, Q * L) : nullptr;
  predict_values_prepare(plan);
  if (T) {
    if (search) HIP_OK(hipFuncSetAttribute((const void*)k_check_reduce<0, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)binLds));
    else HIP_OK(hipFuncSetAttribute((const void*)k_check_reduce<0, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)binLds));
  }
  LaunchCount launched{launches};
  for (int64_t ch = 0; ch < cp.chunks; ++ch) {
    a.chunk0 = ch * C; a.chunkRows = std::min<int64_t>(C, r.nT - a.chunk0);
    predict_values_launch(stream, plan, chunk_grid(a), a); launched();
    p.row0 = a.chunk0; p.rows = a.chunkRows;
    const dim3 grid((unsigned)((p.rows + SP_SLAB - 1) / SP_SLAB), (unsigned)((r.S + SP_BLOCK - 1) / SP_BLOCK));
    if (link) hipLaunchKernelGGL((k_check_reduce<1, false, false>), grid, dim3(SP_BLOCK), 0, stream, p);
    else if (!T) hipLaunchKernelGGL((k_check_reduce<0, false, false>), grid, dim3(SP_BLOCK), 0, stream, p);
    else if (search) hipLaunchKernelGGL((k_check_reduce<0, true, true>), grid, dim3(SP_BLOCK), binLds, stream, p);
    else hipLaunchKernelGGL((k_check_reduce<0, true, false>), grid, dim3(SP_BLOCK), binLds, stream, p);
    launched();
    const int64_t m = r.S + (T ? (int64_t)(T + 1) * r.S : 0);
    hipLaunchKernelGGL(k_check_fold, dim3((unsigned)std::min<int64_t>(GRID_MAX, (m + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, p); launched();
  }
  hipLaunchKernelGGL(k_check_finish, dim3((unsigned)std::min<int64_t>(GRID_MAX, (r.S + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, p); launched();
  sum.run(stream, launched, p.out, (int64_t)L, 0, mean, m2, quantiles, (int64_t)L);
  if (mean) HIP_OK(hipMemcpyAsync(c.mean, mean, L * 8, hipMemcpyDeviceToHost, stream));
  if (m2) HIP_OK(hipMemcpyAsync(c.m2, m2, L * 8, hipMemcpyDeviceToHost, stream));
  if (Q) HIP_OK(hipMemcpyAsync(c.quantiles, quantiles, Q * L * 8, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipMemcpyAsync(c.draws, p.out, L * S * 8, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  r.info[0] = plan.staged ? 1 : 2; r.info[1] = C; r.info[2] = cp.chunks; r.info[3] = launched.mine;
  r.info[4] = buf.bytes; r.info[5] = r.S; r.info[6] = c.T; r.info[7] = c.zeroSlabs;
}
