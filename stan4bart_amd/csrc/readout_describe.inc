// Per-row description of the posterior over the pooled draws (s4b_predict_describe; DESIGN.md 5.17): everything that is a function of ONE row's draws in
// sorted order x(0) <= ... <= x(S-1) — the type-7 quantiles and the median, the shortest window of m draws (the highest-density interval) for up to
// DS_MASS_MAX counts m, the draws strictly above and strictly below up to DS_THR_MAX thresholds, and the median absolute deviation.  x is
// k_predict_values' v (one arm) or k_contrast_values' d (two arms).
// Included by dev_hip.hip inside namespace s4b, after readout_curves.inc: the value kernels, the chunked scratch, the LDS sort, the type-7 read and
// the call scaffold are dev_readout.inc's, dev_quantile.inc's and dev_contrast.inc's.  New here is what is read from the sorted row besides the quantiles.
// Per chunk of C rows (chunk_plan) two launches:
//   k_predict_values<STAGED> / k_contrast_values<STAGED>   unchanged: the chunk's values row-major in the scratch.
//   k_row_describe    k_row_quantiles' shape: 256 threads, R = max(1, 4096 / Sp) rows of Sp padded keys in LDS, qt_sort_rows.  From the sorted segments:
//       quantiles     qt_type7_rows, unchanged: predict_quantiles' / predict_contrast's bits.
//       median        type 7 at 0.5 (g is 0 or exactly 0.5), a thread per row, kept in med[R] behind the keys for the MAD.
//       hdi           a wave per row (rows wave, wave + 4, ...), the lanes stride over the windows j = 0 .. S - m and keep the lexicographic minimum of
//                     (x(j + m - 1) - x(j), j); wave_argmin's xor butterfly on the pair.  No barrier inside, no atomics.
//       counts        a lane per (row, threshold): two binary searches with DOUBLE compares (the key order is consistent with the double order; -0.0 and
//                     +0.0 are one value to a compare).
//       mad           LAST, it destroys the sorted row: behind a barrier every real key becomes qt_key(|x - median|) in place (the padding stays above
//                     every key), qt_sort_rows a second time, type 7 at 0.5.
// LDS: the sort's bytes + 8 R (128 KiB + 8 B at S = 16384, 64 KiB at S = 1).  No atomics, no data-dependent order: the sorted row alone determines
// every output, whatever the chunking, the route, the sampler kind, R or the order of the peers.
constexpr int DS_MASS_MAX = 8;             // hdi counts per call at most
constexpr int DS_THR_MAX = 32;             // thresholds per call at most

struct DescribeDev : QuantileDev {
  double* median; double* hdi; int32_t* hdiStart;          // [nT], [nMass x 2 x nT], [nMass x nT]
  int32_t* nAbove; int32_t* nBelow; double* mad;           // [nThr x nT], [nThr x nT], [nT]
  const double* thr;                                       // [nThr]
  int nMass, nThr;
  int32_t hdiCount[DS_MASS_MAX];
};

// type 7 at 0.5 of the sorted segment x(0 .. S-1): g = h - floor(h) is 0 (odd S: x(lo) itself) or 0.5 (the product is exact)
__device__ __forceinline__ double ds_median(const uint64_t* seg, int64_t S) {
  const double h = 0.5 * (double)(S - 1);
  const int64_t lo = min((int64_t)floor(h), S - 1), hi = min(lo + 1, S - 1);
  const double g = h - (double)lo;
  const double xl = qt_value(seg[lo]), xh = qt_value(seg[hi]);
  return g == 0.0 ? xl : xl + g * (xh - xl);
}

__global__ __launch_bounds__(QT_BLOCK) void k_row_describe(DescribeDev a) {
  extern __shared__ __align__(16) unsigned char ds_lds[];
  uint64_t* key = (uint64_t*)ds_lds;                                               // [R][Sp]
  const int tid = threadIdx.x, Sp = a.Sp, R = a.R, N = R * Sp;
  double* med = (double*)(key + N);                                                // [R]
  const int shift = 31 - __clz(Sp);                                                // Sp = 1 << shift
  const int64_t S = a.S, row0 = (int64_t)blockIdx.x * R;                           // first row of the workgroup inside the chunk
  const int rows = (int)min((int64_t)R, a.chunkRows - row0);                       // the rows of this workgroup that exist
  const size_t nT = (size_t)a.nT, g0 = (size_t)(a.chunk0 + row0);                  // g0: the workgroup's first row among all rows
  for (int e = tid; e < N; e += QT_BLOCK) {
    const int r = e >> shift, j = e & (Sp - 1);
    key[e] = (j < S && r < rows) ? qt_key(a.vals[(size_t)(row0 + r) * (size_t)S + (size_t)j]) : ~0ull;
  }
  __syncthreads();
  qt_sort_rows(key, N, Sp);
  if (a.quantiles) qt_type7_rows(a, key, row0);
  // ---- the median, a thread per row
  for (int r = tid; r < rows; r += QT_BLOCK) {
    const double m = ds_median(key + (size_t)r * Sp, S);
    med[r] = m;
    if (a.median) a.median[g0 + r] = m;
  }
  // ---- the shortest window of m draws, a wave per row: the lowest j among the windows of the smallest width
  if (a.hdi || a.hdiStart) {
    const int lane = tid & 63;
    for (int r = tid >> 6; r < rows; r += QT_BLOCK / 64) {
      const uint64_t* seg = key + (size_t)r * Sp;
      for (int c = 0; c < a.nMass; ++c) {
        const int m = a.hdiCount[c], windows = (int)S - m + 1;
        double best = __longlong_as_double(0x7ff0000000000000ll);                  // a lane without a window: +inf at the highest index, it loses every tie
        int at = 0x7fffffff;
        for (int j = lane; j < windows; j += 64) {
          const double w = qt_value(seg[j + m - 1]) - qt_value(seg[j]);
          if (j == lane || w < best) { best = w; at = j; }                         // (ascending j: an equal width later on does not replace)
        }
        wave_argmin(best, at);
        if (lane == 0) {
          if (a.hdi) {
            a.hdi[(size_t)(2 * c) * nT + g0 + r] = qt_value(seg[at]);
            a.hdi[(size_t)(2 * c + 1) * nT + g0 + r] = qt_value(seg[at + m - 1]);
          }
          if (a.hdiStart) a.hdiStart[(size_t)c * nT + g0 + r] = at;
        }
      }
    }
  }
  // ---- the draws strictly above and strictly below a threshold, a lane per (row, threshold)
  if (a.nAbove || a.nBelow) {
    for (int e = tid; e < rows * a.nThr; e += QT_BLOCK) {
      const int r = e % rows, t = e / rows;                                        // consecutive threads: consecutive rows of one threshold
      const uint64_t* seg = key + (size_t)r * Sp;
      const double th = a.thr[t];
      int lo = 0, hi = (int)S;                                                     // the first index whose draw is not below the threshold
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (qt_value(seg[mid]) < th) lo = mid + 1; else hi = mid; }
      const int below = lo;
      hi = (int)S;                                                                 // the first index whose draw is above it (at or behind `below`)
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (qt_value(seg[mid]) > th) hi = mid; else lo = mid + 1; }
      if (a.nBelow) a.nBelow[(size_t)t * nT + g0 + r] = below;
      if (a.nAbove) a.nAbove[(size_t)t * nT + g0 + r] = (int)S - lo;
    }
  }
  // ---- the median absolute deviation: the sorted row is given up
  if (a.mad) {
    __syncthreads();                                                               // every read of the sorted row above is done, med[] is written
    for (int e = tid; e < N; e += QT_BLOCK) {
      const int r = e >> shift, j = e & (Sp - 1);
      if (j < S && r < rows) key[e] = qt_key(fabs(qt_value(key[e]) - med[r]));
    }
    __syncthreads();
    qt_sort_rows(key, N, Sp);
    for (int r = tid; r < rows; r += QT_BLOCK) a.mad[g0 + r] = ds_median(key + (size_t)r * Sp, S);
  }
}

// the plan alone (every output NULL), else uploads, two launches per chunk of rows, one download per output — on `stream`, everything allocated here
// freed here (summary_run's discipline)
static void describe_run(hipStream_t stream, int P, const DescribeCall& c, int64_t& launches) {
  const ContrastCall& ar = c.arms;
  const bool two = c.nArms == 2;
  bool walks = true;
  SummaryCall r = two ? contrast_rows(ar, walks) : ar.rows;
  const ReadoutPlan plan = readout_plan(r, 0, two ? 8 : 4, false);
  const ChunkPlan cp = chunk_plan(r.nT, r.S, ar.scratchBytes, QT_SCRATCH_DEFAULT, 1, 64);
  const size_t lds = cp.sortLds + (size_t)8 * (size_t)cp.R;
  const int route = !walks ? 0 : plan.staged ? 1 : 2;
  r.info[0] = route; r.info[1] = cp.C; r.info[2] = cp.chunks; r.info[3] = 0; r.info[4] = 0; r.info[5] = r.S;
  r.info[6] = ((int64_t)cp.R << 32) | (int64_t)cp.Sp; r.info[7] = (int64_t)lds;
  if (!c.quantiles && !c.median && !c.hdi && !c.hdiStart && !c.nAbove && !c.nBelow && !c.mad) return;          // the query: the plan, nothing launched
  CallBuffers buf(stream);
  const size_t nT = (size_t)r.nT, S = (size_t)r.S, Q = (size_t)ar.Q, M = (size_t)c.nMass, T = (size_t)c.nThr;
  ContrastDev a{};
  if (two) contrast_upload(buf, a, ar, r, P, plan); else buf.upload_rows(a, r, P, plan.stageNodes);
  a.vals = buf.alloc<double>(nullptr, (size_t)cp.C * S);
  a.Sp = cp.Sp; a.R = cp.R;
  DescribeDev d{};
  if (c.quantiles) { a.probs = buf.alloc(ar.probs, Q); a.quantiles = buf.alloc<double>(nullptr, Q * nT); a.Q = ar.Q; }
  if (c.median) d.median = buf.alloc<double>(nullptr, nT);
  if (c.hdi) d.hdi = buf.alloc<double>(nullptr, M * 2 * nT);
  if (c.hdiStart) d.hdiStart = buf.alloc<int32_t>(nullptr, M * nT);
  if (c.nAbove) d.nAbove = buf.alloc<int32_t>(nullptr, T * nT);
  if (c.nBelow) d.nBelow = buf.alloc<int32_t>(nullptr, T * nT);
  if (c.mad) d.mad = buf.alloc<double>(nullptr, nT);
  if (T) d.thr = buf.alloc(c.thresholds, T);
  d.nMass = c.nMass; d.nThr = c.nThr;
  for (int m = 0; m < c.nMass; ++m) d.hdiCount[m] = c.hdiCount[m];
  arm_values_prepare(plan, two);
  HIP_OK(hipFuncSetAttribute((const void*)k_row_describe, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  LaunchCount launched{launches};
  for (int64_t ch = 0; ch < cp.chunks; ++ch) {
    a.chunk0 = ch * cp.C; a.chunkRows = std::min<int64_t>(cp.C, r.nT - a.chunk0);
    arm_values_launch(stream, plan, chunk_grid(a), a, two); launched();
    static_cast<QuantileDev&>(d) = a;          // the rows, the scratch, the chunk, the probs
    hipLaunchKernelGGL(k_row_describe, dim3((unsigned)((a.chunkRows + cp.R - 1) / cp.R)), dim3(QT_BLOCK), lds, stream, d); launched();
  }
  if (c.quantiles) HIP_OK(hipMemcpyAsync(c.quantiles, a.quantiles, Q * nT * 8, hipMemcpyDeviceToHost, stream));
  if (c.median) HIP_OK(hipMemcpyAsync(c.median, d.median, nT * 8, hipMemcpyDeviceToHost, stream));
  if (c.hdi) HIP_OK(hipMemcpyAsync(c.hdi, d.hdi, M * 2 * nT * 8, hipMemcpyDeviceToHost, stream));
  if (c.hdiStart) HIP_OK(hipMemcpyAsync(c.hdiStart, d.hdiStart, M * nT * 4, hipMemcpyDeviceToHost, stream));
  if (c.nAbove) HIP_OK(hipMemcpyAsync(c.nAbove, d.nAbove, T * nT * 4, hipMemcpyDeviceToHost, stream));
  if (c.nBelow) HIP_OK(hipMemcpyAsync(c.nBelow, d.nBelow, T * nT * 4, hipMemcpyDeviceToHost, stream));
  if (c.mad) HIP_OK(hipMemcpyAsync(c.mad, d.mad, nT * 8, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  r.info[3] = launched.mine; r.info[4] = buf.bytes;
}
