// Per-draw weighted least squares of the rows' values on a small design, summarised over the draws (s4b_predict_projection; DESIGN.md 5.13): for rows
// i < n with the design A [n x K], K <= PJ_COLUMNS_MAX, and weights w_i >= 0
//     G(j,j') = sum_i w_i A(i,j) A(i,j'),   b(j,k) = sum_i w_i A(i,j) x(i,k),   s(k) = sum_i w_i x(i,k),   t(k) = sum_i w_i x(i,k)^2,
//     x = k_predict_values' v (one arm) or k_contrast_values' d (two arms),
//     beta(.,k) = G^-1 b(.,k) (Cholesky),   rss(k) = t(k) - sum_j beta(j,k) b(j,k),   tss(k) = t(k) - s(k)^2 / W,   r2(k) = 1 - rss(k) / tss(k),
// and per coefficient and for r2 the mean, m2, type-7 quantiles and the share of the draws above a threshold.
// Included by dev_hip.hip inside namespace s4b, after dev_groups.inc: the value kernels, the chunked scratch, the LDS sort, the call scaffold and the
// summary over the draws (k_level_rows, k_row_quantiles, unchanged) are dev_readout.inc's, dev_quantile.inc's, dev_contrast.inc's and dev_groups.inc's.
// New here is the skinny product A' W X over the chunk's values and the solve.
//
// THE ORDER OF THE ADDITIONS (include/stan4bart_amd.h states it, tests/projection_cases.py models it): slabs are the GLOBAL blocks of PJ_SLAB rows — a
// chunk starts on a multiple of PJ_SLAB, so a slab never depends on the chunking.  With wx = w_i x(i,k) (x(i,k) itself without weights) a term of b is
// A(i,j) wx, of s is wx, of t is wx x(i,k).  Every moment is the left fold, over the slabs in ascending order, of the slab's partial; a partial is the
// left fold, over the slab's rows in row order, of the terms, begun from +0; the first partial of the fold over the slabs is taken as it is.  A term and
// the addition that takes it in may contract to one fused multiply-add.  G is formed by the same kernels with the design's own columns as the values: G(j,j') = sum_i A(i,j) (w_i
// A(i,j')), of which the factorisation reads j >= j'.
//   k_proj_reduce<KT>   one workgroup (a wave) per slab and block of PJ_BLOCK draws, a draw per lane: src[r ld + k] is read coalesced across the wave,
//                       once.  The design is padded to rows of KT = 8, 16 or 32 doubles, zero-filled (one aligned row of 64, 128 or 256 bytes): lane
//                       l < KT loads entry l of the row — one coalesced load per row — and v_readlane hands entry j to the whole wave as a scalar
//                       operand of the multiply-add; w[r] is a scalar load.  The loads of PJ_AHEAD = 8 rows are issued together, so a wave waits
//                       for memory once per 8 rows, not once per row (with one row in flight the kernel ran at 0.45 TB/s: DESIGN.md 5.13).  A lane
//                       keeps KT + 2 sums in registers (68 VGPRs of doubles at KT = 32) and stores the slab's partials part[slab][K + 2][cols],
//                       coalesced.
//   k_proj_fold         a thread per (j, k): the running total (the first slab's partial as it is in the call's first piece) plus this piece's
//                       partials in slab order.
//   k_proj_solve        after the last chunk.  Every workgroup (one wave) factors G = L L' in LDS (K <= 32: a row per lane, column by column; the
//                       pivot d_j = G(j,j) - sum_p L(j,p)^2 is deficient where not d_j > tol G(j,j)), then a thread per draw runs the two
//                       substitutions in a column of LDS of its own — b(., k) is read with stride S, coalesced across the lanes — and forms rss, tss
//                       and r2 into the matrix [(K + 1) x S] (coefficients, then r2).  A deficient design: NaN everywhere, and the rows of the matrix
//                       are marked empty, so that k_level_rows answers NaN in every summary as it does for a level without rows.
//   k_level_rows, k_row_quantiles   unchanged, over the [(K + 1) x S] matrix as K + 1 levels of unit weight, statistic 0.
// PJ_SLAB = 128.  A slab writes (K + 2) / PJ_SLAB of what it reads — at K = 32 a quarter (64 rows: half, 256 rows: an eighth) — and the partials take
// that share of the chunk's scratch in device memory; at 100 pooled draws a chunk of 83 840 rows is 1 310 waves (256 rows: 656, fewer than the 1 024
// SIMDs of an MI355X), each of which has its loads to itself, so the shorter slab keeps the memory side busier where the draws are few.  Blocking the
// columns instead of the template (8 columns per pass) would re-read the chunk's values K / 8 times.  No LDS in the reduce and the fold, no
// floating-point atomics, no data-dependent order.  Device memory beyond the value kernel's: DESIGN.md 5.13 (the padded design 8 n KT, the weights,
// the partials, the totals and the matrix: nothing grows with n x S beyond the chunk).
constexpr int PJ_SLAB = 128;                     // rows per slab: the unit of the fold, part of the interface
constexpr int PJ_BLOCK = 64;                     // threads per workgroup of k_proj_reduce: one wave, a draw per lane
constexpr int PJ_COLUMNS_MAX = 32;               // S4B_PROJECTION_COLUMNS_MAX
constexpr int PJ_SOLVE_BLOCK = 64;               // threads per workgroup of k_proj_solve: one wave, a draw per lane
constexpr int PJ_AHEAD = 8;                      // rows of a slab whose loads k_proj_reduce keeps in flight together

struct ProjDev {
  const double* src; int64_t ld, cols;           // the values: src[r ld + k], k < cols (the chunk's scratch with ld = cols = S; the padded design with ld = KT, cols = K)
  const double* design; const double* w;         // [nT x KT] zero-padded rows, [nT] or NULL (every weight 1)
  double* part; double* tot;                     // [slabs of a piece][K + 2][cols], [K + 2][cols]
  int64_t row0, rows;                            // the piece's first row among all rows (a multiple of PJ_SLAB) and its rows
  int K, first;                                  // first: the call's first piece (the running total is not read)
};

// entry j of a double that lives one per lane, as a wave-uniform value
__device__ __forceinline__ double pj_lane(double v, int j) {
  const long long q = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)q, j), hi = __builtin_amdgcn_readlane((int)(q >> 32), j);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

template <int KT>
__global__ __launch_bounds__(PJ_BLOCK) void k_proj_reduce(ProjDev a) {
  const int lane = threadIdx.x;
  const int64_t k = (int64_t)blockIdx.y * PJ_BLOCK + lane;
  const bool mine = k < a.cols;                                                    // (the other lanes stay: lanes 0 .. KT - 1 carry the design row)
  const int64_t r0 = (int64_t)blockIdx.x * PJ_SLAB, g0 = a.row0 + r0;              // the slab's first row inside the piece and among all rows
  const int rows = (int)min((int64_t)PJ_SLAB, a.rows - r0);
  const double* __restrict__ des = a.design + (size_t)g0 * KT + (size_t)(lane & (KT - 1));          // lane l < KT: entry l of a row
  const double* __restrict__ w = a.w ? a.w + g0 : nullptr;                         // (the same for every lane: scalar loads)
  const double* __restrict__ v = a.src + (size_t)r0 * (size_t)a.ld + (size_t)(mine ? k : a.cols - 1);
  double b[KT], s = 0.0, t = 0.0;
#pragma unroll
  for (int j = 0; j < KT; ++j) b[j] = 0.0;
  for (int r = 0; r < rows; r += PJ_AHEAD) {
    double xs[PJ_AHEAD], ds[PJ_AHEAD], ws[PJ_AHEAD];
#pragma unroll
    for (int u = 0; u < PJ_AHEAD; ++u) {                                           // the loads of PJ_AHEAD rows in flight together (past the slab's end: its last row again)
      const int q = min(r + u, rows - 1);
      xs[u] = v[(size_t)q * (size_t)a.ld];
      ds[u] = des[(size_t)q * KT];
      ws[u] = w ? w[q] : 1.0;
    }
#pragma unroll
    for (int u = 0; u < PJ_AHEAD; ++u) {
      if (r + u < rows) {                                                          // (the same for every lane)
        const double x = xs[u], wx = w ? ws[u] * x : x;
        s += wx; t += wx * x;
#pragma unroll
        for (int j = 0; j < KT; ++j) b[j] += pj_lane(ds[u], j) * wx;
      }
    }
  }
  if (!mine) return;
  double* out = a.part + (size_t)blockIdx.x * (size_t)(a.K + 2) * (size_t)a.cols + (size_t)k;
#pragma unroll
  for (int j = 0; j < KT; ++j) if (j < a.K) out[(size_t)j * (size_t)a.cols] = b[j];
  out[(size_t)a.K * (size_t)a.cols] = s;
  out[(size_t)(a.K + 1) * (size_t)a.cols] = t;
}

__global__ __launch_bounds__(BLOCK) void k_proj_fold(ProjDev a) {
  const int64_t m = (int64_t)(a.K + 2) * a.cols, slabs = (a.rows + PJ_SLAB - 1) / PJ_SLAB;
  for (int64_t x = (int64_t)blockIdx.x * BLOCK + threadIdx.x; x < m; x += (int64_t)gridDim.x * BLOCK) {
    int64_t sl = 0;
    double acc;
    if (a.first) { acc = a.part[(size_t)x]; sl = 1; }                              // the first slab's partial as it is
    else acc = a.tot[(size_t)x];                                                   // what the piece before left
#pragma unroll 8
    for (; sl < slabs; ++sl) acc += a.part[(size_t)sl * (size_t)m + (size_t)x];
    a.tot[(size_t)x] = acc;
  }
}

struct ProjSolveDev {
  const double* gram; const double* mom;         // [K + 2][K]: G(j,j') at gram[j K + j'], read for j >= j'; [K + 2][S]: b, s, t
  double* out;                                   // [(K + 1) x S]: the coefficients, then r2
  int64_t* levelStart; int64_t* flag;            // [K + 2]: emptied where the design is deficient (k_level_rows then answers NaN); [1]: 1 deficient, 0 not
  int64_t S; int K; double W, tol;
};

__global__ __launch_bounds__(PJ_SOLVE_BLOCK) void k_proj_solve(ProjSolveDev a) {
  __shared__ double L[PJ_COLUMNS_MAX][PJ_COLUMNS_MAX + 1];
  __shared__ double Y[PJ_COLUMNS_MAX][PJ_SOLVE_BLOCK];                             // Y[j][tid]: a thread's own column, the substitutions' work space
  __shared__ int bad;
  const int K = a.K, tid = threadIdx.x;
  const int64_t S = a.S;
  if (tid == 0) bad = 0;
  for (int j = 0; j < K; ++j) {                                                    // column j of the factor: the pivot, then a row per lane
    if (tid == j) {
      const double g = a.gram[(size_t)j * K + j];
      double d = g;
      for (int p = 0; p < j; ++p) d -= L[j][p] * L[j][p];
      if (!(d > a.tol * g)) bad = 1;                                               // (a NaN is deficient too)
      L[j][j] = sqrt(d);
    }
    __syncthreads();
    if (tid > j && tid < K) {
      double e = a.gram[(size_t)tid * K + j];
      for (int p = 0; p < j; ++p) e -= L[tid][p] * L[j][p];
      L[tid][j] = e / L[j][j];
    }
    __syncthreads();
  }
  const bool deficient = bad != 0;                                                 // (the same in every workgroup: each factors the same G in the same order)
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  if (blockIdx.x == 0 && tid == 0) a.flag[0] = deficient ? 1 : 0;
  if (deficient && blockIdx.x == 0 && tid < K + 2) a.levelStart[tid] = 0;         // every row of the matrix is a level without rows
  for (int64_t k = (int64_t)blockIdx.x * PJ_SOLVE_BLOCK + tid; k < S; k += (int64_t)gridDim.x * PJ_SOLVE_BLOCK) {
    double* o = a.out + (size_t)k;                                                 // o[j S]: this draw's column of the matrix
    if (deficient) { for (int j = 0; j <= K; ++j) o[(size_t)j * (size_t)S] = nan; continue; }
    const double* b = a.mom + (size_t)k;
    for (int j = 0; j < K; ++j) {                                                  // L y = b
      double y = b[(size_t)j * (size_t)S];
      for (int p = 0; p < j; ++p) y -= L[j][p] * Y[p][tid];
      Y[j][tid] = y / L[j][j];
    }
    for (int j = K - 1; j >= 0; --j) {                                             // L' beta = y
      double y = Y[j][tid];
      for (int p = j + 1; p < K; ++p) y -= L[p][j] * Y[p][tid];
      Y[j][tid] = y / L[j][j];
    }
    const double s = b[(size_t)K * (size_t)S], t = b[(size_t)(K + 1) * (size_t)S];
    double rss = t;
    for (int j = 0; j < K; ++j) { const double c = Y[j][tid]; o[(size_t)j * (size_t)S] = c; rss -= c * b[(size_t)j * (size_t)S]; }
    const double tss = t - s * s / a.W;
    o[(size_t)K * (size_t)S] = tss == 0.0 ? nan : 1.0 - rss / tss;
  }
}

// uploads, the design's own moments, per chunk the value kernel, the reduce and the fold, then the solve, the summary kernels and the downloads — on
// `stream`, everything allocated here freed here (summary_run's discipline)
static void projection_run(hipStream_t stream, int P, const ProjectionCall& c, int64_t& launches) {
  const ContrastCall& ar = c.arms;
  const bool two = c.nArms == 2;
  bool walks = true;
  SummaryCall r = two ? contrast_rows(ar, walks) : ar.rows;
  const ReadoutPlan plan = readout_plan(r, 0, two ? 8 : 4, false);
  const ChunkPlan cp = chunk_plan(r.nT, r.S, ar.scratchBytes, QT_SCRATCH_DEFAULT, 1, PJ_SLAB);          // whole slabs
  CallBuffers buf(stream);
  const size_t nT = (size_t)r.nT, S = (size_t)r.S, Q = (size_t)ar.Q, K = (size_t)c.K, L = K + 1;
  const int KT = c.K <= 8 ? 8 : c.K <= 16 ? 16 : 32;
  const int64_t C = cp.C, slabsMax = (C + PJ_SLAB - 1) / PJ_SLAB;
  // the design in rows of KT doubles, zero-filled
  std::vector<double> padded;
  if ((int)K != KT) {
    padded.assign(nT * (size_t)KT, 0.0);
    for (size_t i = 0; i < nT; ++i) std::copy(c.design + i * K, c.design + (i + 1) * K, padded.begin() + i * (size_t)KT);
  }
  ContrastDev a{};
  if (two) contrast_upload(buf, a, ar, r, P, plan); else buf.upload_rows(a, r, P, plan.stageNodes);
  a.vals = buf.alloc<double>(nullptr, (size_t)C * S);
  ProjDev p{};
  p.design = buf.alloc((int)K != KT ? padded.data() : c.design, nT * (size_t)KT);
  if (c.rowWeights) p.w = buf.alloc(c.rowWeights, nT);
  p.part = buf.alloc<double>(nullptr, (size_t)slabsMax * (K + 2) * std::max(S, K));
  p.K = c.K;
  double* gram = buf.alloc<double>(nullptr, (K + 2) * K);
  double* mom = buf.alloc<double>(nullptr, (K + 2) * S);
  ProjSolveDev sv{};
  sv.gram = gram; sv.mom = mom; sv.out = buf.alloc<double>(nullptr, L * S);
  sv.flag = buf.alloc<int64_t>(nullptr, 1);
  sv.S = r.S; sv.K = c.K; sv.W = c.W; sv.tol = c.tol;
  LevelsSummary sum;          // the matrix's K + 1 rows as levels of unit weight, whose starts the solve empties where the design is deficient
  sum.prepare(buf, cp, r.S, ar.probs, ar.Q, (int64_t)L);
  sv.levelStart = const_cast<int64_t*>(sum.g.levelStart);
  GroupsDev& g = sum.g;       // a threshold and pAbove beside mean and m2: k_level_rows is launched here, over the matrix at once
  g.lev = sv.out; g.L = (int64_t)L; g.hasThreshold = c.hasThreshold; g.threshold = c.threshold;
  if (c.mean) g.mean = buf.alloc<double>(nullptr, L);
  if (c.m2) g.m2 = buf.alloc<double>(nullptr, L);
  if (c.pAbove) g.pAbove = buf.alloc<double>(nullptr, L);
  double* quantiles = Q ? buf.alloc<double>(nullptr, Q * L) : nullptr;
  arm_values_prepare(plan, two);
  LaunchCount launched{launches};
  // the reduce and the fold of one piece of rows: p.src, p.ld, p.cols, p.tot, p.row0, p.rows, p.first are set
  auto moments = [&]() {
    const dim3 grid((unsigned)((p.rows + PJ_SLAB - 1) / PJ_SLAB), (unsigned)((p.cols + PJ_BLOCK - 1) / PJ_BLOCK));
    if (KT == 8) hipLaunchKernelGGL(k_proj_reduce<8>, grid, dim3(PJ_BLOCK), 0, stream, p);
    else if (KT == 16) hipLaunchKernelGGL(k_proj_reduce<16>, grid, dim3(PJ_BLOCK), 0, stream, p);
    else hipLaunchKernelGGL(k_proj_reduce<32>, grid, dim3(PJ_BLOCK), 0, stream, p);
    launched();
    const int64_t m = (int64_t)(p.K + 2) * p.cols;
    hipLaunchKernelGGL(k_proj_fold, dim3((unsigned)std::min<int64_t>(GRID_MAX, (m + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, p); launched();
  };
  // G, once per call: the design's own columns as the values, in the pieces the chunks are
  for (int64_t ch = 0; ch < cp.chunks; ++ch) {
    p.row0 = ch * C; p.rows = std::min<int64_t>(C, r.nT - p.row0); p.first = ch == 0;
    p.src = p.design + (size_t)p.row0 * (size_t)KT; p.ld = KT; p.cols = c.K; p.tot = gram;
    moments();
  }
  for (int64_t ch = 0; ch < cp.chunks; ++ch) {
    a.chunk0 = ch * C; a.chunkRows = std::min<int64_t>(C, r.nT - a.chunk0);
    arm_values_launch(stream, plan, chunk_grid(a), a, two); launched();
    p.row0 = a.chunk0; p.rows = a.chunkRows; p.first = ch == 0;
    p.src = a.vals; p.ld = r.S; p.cols = r.S; p.tot = mom;
    moments();
  }
  hipLaunchKernelGGL(k_proj_solve, dim3((unsigned)std::min<int64_t>(GRID_MAX, (r.S + PJ_SOLVE_BLOCK - 1) / PJ_SOLVE_BLOCK)), dim3(PJ_SOLVE_BLOCK), 0, stream, sv); launched();
  hipLaunchKernelGGL(k_level_rows, dim3((unsigned)((L + BLOCK / 64 - 1) / (BLOCK / 64))), dim3(BLOCK), 0, stream, g); launched();
  if (Q) sum.run(stream, launched, sv.out, (int64_t)L, 0, nullptr, nullptr, quantiles, (int64_t)L);
  int64_t flag = 0;
  HIP_OK(hipMemcpyAsync(c.coef, sv.out, K * S * 8, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipMemcpyAsync(c.r2, sv.out + K * S, S * 8, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipMemcpyAsync(&flag, sv.flag, 8, hipMemcpyDeviceToHost, stream));
  if (c.mean) HIP_OK(hipMemcpyAsync(c.mean, g.mean, L * 8, hipMemcpyDeviceToHost, stream));
  if (c.m2) HIP_OK(hipMemcpyAsync(c.m2, g.m2, L * 8, hipMemcpyDeviceToHost, stream));
  if (c.pAbove) HIP_OK(hipMemcpyAsync(c.pAbove, g.pAbove, L * 8, hipMemcpyDeviceToHost, stream));
  if (Q) HIP_OK(hipMemcpyAsync(c.quantiles, quantiles, Q * L * 8, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  r.info[0] = !walks ? 0 : plan.staged ? 1 : 2; r.info[1] = C; r.info[2] = cp.chunks; r.info[3] = launched.mine;
  r.info[4] = buf.bytes; r.info[5] = r.S; r.info[6] = flag; r.info[7] = c.K;
}

