// Per-row quantiles of the kept draws' predictions, pooled over several samplers (s4b_predict_quantiles; DESIGN.md 5.7).
// Included by dev_hip.hip inside namespace s4b, after dev_summary.inc and, through it, dev_readout.inc: the walk, the staging, the linear part, the out-of-line Phi and the route are there.
// Shared with every chunked read-out behind it (the host side, below the kernels): LaunchCount, ChunkPlan / chunk_plan (rows per chunk, padded draws, rows per
// sort workgroup), chunk_grid (segments of draws), predict_values_prepare / _launch and row_quantiles_prepare / _launch.
//
// The host hands down ONE pooled description (QuantileCall.rows: the kept draws of the sampler and its peers concatenated, S draws) and loops over
// chunks of C rows.  Per chunk two launches on the sampler's stream:
//   k_predict_values<STAGED>   v(i,k) of predict_summary (the same z, the same order of the additions, link 0 / 1) for the rows of the chunk, written
//                              ROW-major into the scratch: vals[(i - chunk0) * S + k].  No Welford pair, no weights, no reduction.  A thread keeps
//                              QT_GROUP consecutive draws in registers and stores them at once: the stores of a thread cover whole 64-byte segments
//                              instead of 8-byte scatters at stride 8 S.  The draws are split over blockIdx.y (segments of segDraws draws, a
//                              multiple of QT_GROUP): no state is carried from draw to draw, so a chunk of few tiles spreads over the device.
//   k_row_quantiles            a workgroup of 256 threads loads R = max(1, 4096 / Sp) rows of S values into LDS as monotone uint64 keys (Sp = S
//                              rounded up to a power of two, every row padded to Sp with keys above every real key), runs ONE bitonic network over all
//                              R * Sp elements stopped at merge size Sp — the direction of a compare-exchange is taken from the index inside the
//                              segment, so every segment comes out ascending on its own — and forms the Q quantiles of each row (R's type 7):
//                                  h = p (S - 1), lo = floor(h), hi = min(lo + 1, S - 1), g = h - lo, q = x(lo) + g (x(hi) - x(lo))      (g = 0: x(lo) itself)
//                              stored prob-major: quantiles[j * n + i].  No atomics, no data-dependent order: two calls return the same bits.
constexpr int QT_GROUP = 8;                // draws a thread of k_predict_values buffers in registers: one 64-byte segment per store group (VGPRs: DESIGN.md 5.7)
constexpr int QT_BLOCK = 256;              // threads per workgroup of k_row_quantiles
constexpr int QT_SORT = 4096;              // elements a sort workgroup holds at least (32 KB of keys)
constexpr int QT_FILL = 256;               // workgroups of k_predict_values a chunk is spread over where it has the draws for it (the compute units of an MI355X)
constexpr int QT_SEG_MIN = 16;             // draws per workgroup at least: the first draw of a segment is staged behind a barrier of its own
constexpr int64_t QT_DRAWS_MAX = 16384;    // pooled draws at most: one row as 8-byte keys in 128 KB of LDS
constexpr int QT_PROBS_MAX = 16;
#ifndef S4B_QT_SCRATCH_MIB
#define S4B_QT_SCRATCH_MIB 64              // measured against 256 and 1024 (DESIGN.md 5.7); a measurement build may set another (tools/quantile_probe.py)
#endif
constexpr int64_t QT_SCRATCH_DEFAULT = (int64_t)S4B_QT_SCRATCH_MIB << 20;   // value scratch of a chunk at most

struct QuantileDev : RowsDev {
  double* vals;              // [C x S], row-major
  const double* probs; double* quantiles;          // [Q], [Q x nT]
  int64_t chunk0, chunkRows, segDraws;          // segDraws: draws per workgroup of k_predict_values, a multiple of QT_GROUP
  int Q, Sp, R;
};

template <bool STAGED>
__global__ __launch_bounds__(PS_BLOCK) void k_predict_values(QuantileDev a) {
  extern __shared__ __align__(16) unsigned char qv_lds[];
  WalkNode* nbuf = (WalkNode*)qv_lds;                                              // [2][stageNodes]
  int32_t* sbuf = (int32_t*)(qv_lds + (size_t)2 * a.stageNodes * sizeof(WalkNode));   // [2][T]: tree starts inside the draw
  const int tid = threadIdx.x, T = a.T;
  const int64_t S = a.S, C = a.chunkRows;
  const int64_t tiles = (C + PS_BLOCK - 1) / PS_BLOCK;

  // the draws of this workgroup (blockIdx.y): the values of different draws share nothing, so a chunk with few tiles still fills the device
  const int64_t k0 = (int64_t)blockIdx.y * a.segDraws, k1 = min(S, k0 + a.segDraws);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r = tile * PS_BLOCK + tid;      // row inside the chunk
    const bool act = r < C;
    const size_t ii = (size_t)(a.chunk0 + (act ? r : C - 1));        // threads beyond the chunk's last row walk that row and store nothing
    const double off = a.offset ? a.offset[ii] : 0.0;
    double* out = a.vals + (size_t)(act ? r : 0) * (size_t)S;
    double grp[QT_GROUP];
#pragma unroll
    for (int u = 0; u < QT_GROUP; ++u) grp[u] = 0.0;
    __syncthreads();                              // the tile before is done with the staging buffers
    if (STAGED) { stage_draw<false>(a, k0, nbuf, sbuf, nullptr); __syncthreads(); }
    for (int64_t k = k0; k < k1; ++k) {
      const int b = (int)((k - k0) & 1);
      // draw k + 1 into the other buffer (last read in draw k - 1, before that draw's barrier)
      if (STAGED && k + 1 < k1) stage_draw<false>(a, k + 1, nbuf + (size_t)(b ^ 1) * a.stageNodes, sbuf + (size_t)(b ^ 1) * T, nullptr);
      double z = response_scale(a, k, walk_all<STAGED>(a, nbuf + (size_t)b * a.stageNodes, sbuf + (size_t)b * T, k, ii));
      if (a.offset) z += off;
      z = add_linear(z, a, k, ii);
      const double v = a.link ? readout_phi(z) : z;
      // ---- draw k into its place of the group (selects, not an indexed array: the group stays in registers); a full group leaves at once
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

// the usual order-preserving map of a double's bits to uint64 (negative: all bits flipped, else the sign bit set) and back
__device__ __forceinline__ uint64_t qt_key(double x) { const uint64_t b = (uint64_t)__double_as_longlong(x); return (b >> 63) ? ~b : b | 0x8000000000000000ull; }
__device__ __forceinline__ double qt_value(uint64_t k) { return __longlong_as_double((long long)((k >> 63) ? k & 0x7fffffffffffffffull : ~k)); }

// one bitonic network over all N = R * Sp keys of a sort workgroup, stopped at merge size Sp: ascending where bit `size` of the index INSIDE the segment
// is clear, which at size = Sp is everywhere.  Every segment of Sp keys comes out ascending on its own.  Called by all QT_BLOCK threads, behind a barrier.
__device__ __forceinline__ void qt_sort_rows(uint64_t* key, int N, int Sp) {
  const int tid = threadIdx.x;
  for (int size = 2; size <= Sp; size <<= 1) {
    for (int j = size >> 1; j > 0; j >>= 1) {
      for (int pr = tid; pr < (N >> 1); pr += QT_BLOCK) {
        const int lo = ((pr & ~(j - 1)) << 1) | (pr & (j - 1)), hi = lo | j;
        const bool up = ((lo & (Sp - 1)) & size) == 0;
        const uint64_t x = key[lo], y = key[hi];
        if ((x > y) == up) { key[lo] = y; key[hi] = x; }
      }
      __syncthreads();
    }
  }
}
// R's type 7 of the sorted rows of a sort workgroup, stored prob-major: quantiles[j * nT + i]
__device__ __forceinline__ void qt_type7_rows(const QuantileDev& a, const uint64_t* key, int64_t row0) {
  const int R = a.R, Sp = a.Sp;
  const int64_t S = a.S;
  for (int e = threadIdx.x; e < R * a.Q; e += QT_BLOCK) {
    const int r = e % R, j = e / R;                                                // consecutive threads: consecutive rows of one prob
    if (row0 + r >= a.chunkRows) continue;
    const double h = a.probs[j] * (double)(S - 1);
    const int64_t lo = min((int64_t)floor(h), S - 1), hi = min(lo + 1, S - 1);
    const double g = h - (double)lo;
    const double xl = qt_value(key[(size_t)r * Sp + lo]), xh = qt_value(key[(size_t)r * Sp + hi]);
    a.quantiles[(size_t)j * (size_t)a.nT + (size_t)(a.chunk0 + row0 + r)] = g == 0.0 ? xl : xl + g * (xh - xl);
  }
}

__global__ __launch_bounds__(QT_BLOCK) void k_row_quantiles(QuantileDev a) {
  extern __shared__ __align__(16) unsigned char qs_lds[];
  uint64_t* key = (uint64_t*)qs_lds;                                               // [R][Sp]
  const int tid = threadIdx.x, Sp = a.Sp, R = a.R, N = R * Sp;
  const int shift = 31 - __clz(Sp);                                                // Sp = 1 << shift
  const int64_t S = a.S, row0 = (int64_t)blockIdx.x * R;                           // first row of the workgroup inside the chunk
  for (int e = tid; e < N; e += QT_BLOCK) {
    const int r = e >> shift, j = e & (Sp - 1);
    key[e] = (j < S && row0 + r < a.chunkRows) ? qt_key(a.vals[(size_t)(row0 + r) * (size_t)S + (size_t)j]) : ~0ull;
  }
  __syncthreads();
  qt_sort_rows(key, N, Sp);
  qt_type7_rows(a, key, row0);
}

// ---- the host side that every chunked read-out shares (DESIGN.md 5.7): the launch count, the chunk plan, a chunk's launch grid, the launches of
// k_predict_values and of k_row_quantiles.  A *_run keeps its own plain loop over the chunks and calls these inside it.

// the launch just made: checked, and counted for the sampler and for the call
struct LaunchCount {
  int64_t& launches; int64_t mine = 0;
  void operator()() { HIP_OK(hipGetLastError()); ++launches; ++mine; }
};

// how a call cuts its rows into chunks and sorts a row of draws: C rows per chunk, Sp = S rounded up to a power of two, R rows per sort workgroup
struct ChunkPlan { int64_t C, chunks; int Sp, R; size_t sortLds; };
// rows per chunk: what the scratch holds (the call's scratch_bytes, at most and by default scratchDefault; perRowDraw values of 8 bytes per row and
// draw), a multiple of `multiple`, at least that, at most all rows
static ChunkPlan chunk_plan(int64_t nT, int64_t S, int64_t scratchBytes, int64_t scratchDefault, int64_t perRowDraw, int64_t multiple) {
  ChunkPlan p;
  const int64_t scratch = scratchBytes > 0 ? std::min(scratchBytes, scratchDefault) : scratchDefault;
  p.C = std::min<int64_t>(nT, std::max<int64_t>(multiple, scratch / (8 * S * perRowDraw) / multiple * multiple));
  p.chunks = (nT + p.C - 1) / p.C;
  p.Sp = 1; while (p.Sp < S) p.Sp <<= 1;
  p.R = std::max(1, QT_SORT / p.Sp);
  p.sortLds = (size_t)8 * (size_t)std::max(p.Sp, QT_SORT);
  return p;
}
// the grid of a value kernel over the chunk a.chunkRows: tiles of PS_BLOCK rows times segments of a.segDraws draws, which is set here
static dim3 chunk_grid(QuantileDev& a) {
  const int wg = (int)std::min<int64_t>((a.chunkRows + PS_BLOCK - 1) / PS_BLOCK, PS_GRID_MAX);
  // segments of draws: enough to reach QT_FILL workgroups, each of at least QT_SEG_MIN draws and a multiple of QT_GROUP (a thread's store groups stay whole)
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>((QT_FILL + wg - 1) / wg, a.S / QT_SEG_MIN));
  a.segDraws = ((a.S + want - 1) / want + QT_GROUP - 1) / QT_GROUP * QT_GROUP;
  return dim3(wg, (unsigned)((a.S + a.segDraws - 1) / a.segDraws));
}
// k_predict_values: once per call the LDS of the staged route, then a launch per chunk (a read-out's own *Dev goes in as its QuantileDev part)
static void predict_values_prepare(const ReadoutPlan& plan) {
  if (plan.staged) HIP_OK(hipFuncSetAttribute((const void*)k_predict_values<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
}
static void predict_values_launch(hipStream_t stream, const ReadoutPlan& plan, dim3 grid, const QuantileDev& a) {
  if (plan.staged) hipLaunchKernelGGL(k_predict_values<true>, grid, dim3(PS_BLOCK), plan.lds, stream, a);
  else hipLaunchKernelGGL(k_predict_values<false>, grid, dim3(PS_BLOCK), 0, stream, a);
}
// k_row_quantiles: once per call its LDS, then a launch over the a.chunkRows rows at a.vals
static void row_quantiles_prepare(const ChunkPlan& cp) {
  HIP_OK(hipFuncSetAttribute((const void*)k_row_quantiles, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cp.sortLds));
}
static void row_quantiles_launch(hipStream_t stream, const ChunkPlan& cp, const QuantileDev& a) {
  hipLaunchKernelGGL(k_row_quantiles, dim3((unsigned)((a.chunkRows + cp.R - 1) / cp.R)), dim3(QT_BLOCK), cp.sortLds, stream, a);
}

// uploads, two launches per chunk of rows, the download — on `stream`, everything allocated here freed here (summary_run's discipline)
static void quantile_run(hipStream_t stream, int P, const QuantileCall& c, int64_t& launches) {
  const SummaryCall& r = c.rows;
  const ReadoutPlan plan = readout_plan(r, 0, 4, false);          // no reduction space; the workgroups are chosen per chunk
  const ChunkPlan cp = chunk_plan(r.nT, r.S, c.scratchBytes, QT_SCRATCH_DEFAULT, 1, 64);
  CallBuffers buf(stream);
  const size_t nT = (size_t)r.nT, S = (size_t)r.S, Q = (size_t)c.Q;
  QuantileDev a{};
  buf.upload_rows(a, r, P, plan.stageNodes);
  a.vals = buf.alloc<double>(nullptr, (size_t)cp.C * S);
  a.probs = buf.alloc(c.probs, Q);
  a.quantiles = buf.alloc<double>(nullptr, Q * nT);
  a.Q = c.Q; a.Sp = cp.Sp; a.R = cp.R;
  predict_values_prepare(plan);
  row_quantiles_prepare(cp);
  LaunchCount launched{launches};
  for (int64_t ch = 0; ch < cp.chunks; ++ch) {
    a.chunk0 = ch * cp.C; a.chunkRows = std::min<int64_t>(cp.C, r.nT - a.chunk0);
    predict_values_launch(stream, plan, chunk_grid(a), a); launched();
    row_quantiles_launch(stream, cp, a); launched();
  }
  HIP_OK(hipMemcpyAsync(c.quantiles, a.quantiles, Q * nT * 8, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  r.info[0] = plan.staged ? 1 : 2; r.info[1] = cp.C; r.info[2] = cp.chunks; r.info[3] = ((int64_t)cp.R << 32) | (int64_t)cp.Sp;
  r.info[4] = r.maxDrawNodes; r.info[5] = launched.mine; r.info[6] = buf.bytes; r.info[7] = r.S;
}
