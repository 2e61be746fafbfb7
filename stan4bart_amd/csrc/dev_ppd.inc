// The posterior predictive read-out over the pooled kept draws (s4b_predict_ppd; DESIGN.md 5.9): prediction intervals for new observations and the
// scores of held-out responses, per row, without the [rows x draws] matrix.
// Included by dev_hip.hip inside namespace s4b, after dev_quantile.inc: the walk, the staging, the chunked value scratch, k_predict_values, the LDS sort
// and the type-7 interpolation are dev_readout.inc's and dev_quantile.inc's; the generator is philox.hpp's.
//
// Per chunk of C rows two launches on the sampler's stream:
//   k_predict_values<STAGED>   UNCHANGED and always with link 0: the scratch holds z(i,k), predict_summary's z.
//   k_ppd_rows                 a workgroup of QT_BLOCK threads owns R = max(1, 4096 / Sp) rows as k_row_quantiles does.  It loads its rows of z into LDS
//                              ONCE (the raw bits of the doubles, padded to Sp per row).  Then
//       y given:   per row, from LDS, in two passes that both recompute l(i,k) (a second array of l would not fit beside 128 KB of keys):
//                      link 0: sd = sigma[k] row_scale[i], r = (y_i - z) / sd, l = (-log(2 pi) / 2 - log sd) - r r / 2
//                      link 1: l = log Phi(z) where y_i = 1, log Phi(-z) where y_i = 0      (Phi at the signed argument: readout_phi, out of line)
//                  pass 1: m = max_k l, sum_k l (lmean = sum / S), sum_k Phi(r) (pit = sum / S, link 0 and asked for only)
//                  pass 2: sum_k exp(l - m) (lpd = m + log(sum) - log S), sum_k (l - lmean)^2 (lm2)
//                  A row belongs to W = max(1, 4 / R) waves (1, 2 or all 4 of the workgroup); lane `lane` of sub-wave `sub` takes the draws
//                  k = 64 sub + lane, + 64 W, ... in ascending order, the lanes of a wave are folded by the xor butterfly (wave_sum / wave_max: a fixed
//                  pairing), the W waves of a row in wave order through 16 doubles of LDS behind the keys.  No atomics: two calls return the same bits.
//       n_probs > 0 (link 0 only): every element is overwritten by the key of y_rep = z + sd e(i,k), e = philox_normal(noise key, row i OF THE CALL,
//                  pooled draw k) formed in registers; then dev_quantile.inc's bitonic network and type 7, exactly as k_row_quantiles runs them.
//                  The scratch is read once and never written by this kernel.
// LDS: 8 max(Sp, 4096) + 128 bytes, at most 128 KB + 128 B of the 160 KB of a compute unit: from Sp = 8192 on (more than 80 KB) one workgroup owns
// a compute unit, four waves, one per SIMD (DESIGN.md 5.9).
constexpr int PP_RED = 16;                 // doubles of reduction space behind the keys: [4 waves][4]

struct PpdDev : QuantileDev {
  const double* y; const double* sigma; const double* rowScale;          // [nT] or NULL; [S] (link 0); [nT] or NULL (= 1)
  double* lpd; double* lmean; double* lm2; double* pit;                  // [nT] each, or NULL
  uint32_t key0, key1;
  int ppdLink;                                                           // the response: 0 continuous, 1 binary.  RowsDev::link stays 0: the scratch holds z
};

// l(i,k) from z; under link 0 the standardised residual is handed back for the PIT
__device__ __forceinline__ double ppd_loglik(int link, double y, double z, double sd, double& r) {
  if (link) { r = 0.0; return log(readout_phi(y > 0.0 ? z : -z)); }
  r = (y - z) / sd;
  return (-0.91893853320467274178 - log(sd)) - 0.5 * (r * r);
}

__global__ __launch_bounds__(QT_BLOCK) void k_ppd_rows(PpdDev a) {
  extern __shared__ __align__(16) unsigned char pp_lds[];
  uint64_t* key = (uint64_t*)pp_lds;                                               // [R][Sp]: first the bits of z, then the keys of y_rep
  const int tid = threadIdx.x, Sp = a.Sp, R = a.R, N = R * Sp;
  double* red = (double*)(pp_lds + (size_t)8 * N);                                 // [4][4]
  const int shift = 31 - __clz(Sp);                                                // Sp = 1 << shift
  const int64_t S = a.S, row0 = (int64_t)blockIdx.x * R;                           // first row of the workgroup inside the chunk
  for (int e = tid; e < N; e += QT_BLOCK) {
    const int r = e >> shift, j = e & (Sp - 1);
    key[e] = (j < S && row0 + r < a.chunkRows) ? (uint64_t)__double_as_longlong(a.vals[(size_t)(row0 + r) * (size_t)S + (size_t)j]) : ~0ull;
  }
  __syncthreads();

  if (a.y) {
    const int wave = tid >> 6, lane = tid & 63, link = a.ppdLink;
    const int W = R >= 4 ? 1 : 4 / R, slots = 4 / W;                               // waves that share a row; rows in flight (R is a power of two)
    const int sub = wave % W, slot = wave / W;
    const bool wantPit = a.pit != nullptr;
    for (int rb = 0; rb < R; rb += slots) {                                        // uniform over the workgroup: the barriers below are met by all
      const int r = rb + slot;
      const bool live = row0 + r < a.chunkRows;
      const size_t i = (size_t)(a.chunk0 + row0 + (live ? r : 0));
      const uint64_t* zr = key + (size_t)r * Sp;
      const double yi = a.y[i], rs = (!link && a.rowScale) ? a.rowScale[i] : 1.0;
      // ---- pass 1: the maximum, the sum of l, the sum of Phi(r)
      double mx = -INFINITY, sl = 0.0, sp = 0.0;
      if (live) for (int64_t k = sub * 64 + lane; k < S; k += 64 * W) {
        double rr;
        const double l = ppd_loglik(link, yi, __longlong_as_double((long long)zr[k]), link ? 1.0 : a.sigma[k] * rs, rr);
        mx = fmax(mx, l); sl += l;
        if (wantPit) sp += readout_phi(rr);
      }
      mx = wave_max(mx); sl = wave_sum(sl); sp = wave_sum(sp);
      if (W > 1) {
        if (lane == 0) { red[wave * 4] = mx; red[wave * 4 + 1] = sl; red[wave * 4 + 2] = sp; }
        __syncthreads();
        mx = red[slot * W * 4]; sl = red[slot * W * 4 + 1]; sp = red[slot * W * 4 + 2];
        for (int w = 1; w < W; ++w) { mx = fmax(mx, red[(slot * W + w) * 4]); sl += red[(slot * W + w) * 4 + 1]; sp += red[(slot * W + w) * 4 + 2]; }
        __syncthreads();
      }
      const double mean = sl / (double)S;
      // ---- pass 2: the shifted exponentials, the squared deviations
      double se = 0.0, q = 0.0;
      if (live) for (int64_t k = sub * 64 + lane; k < S; k += 64 * W) {
        double rr;
        const double l = ppd_loglik(link, yi, __longlong_as_double((long long)zr[k]), link ? 1.0 : a.sigma[k] * rs, rr);
        const double d = l - mean;
        se += exp(l - mx); q += d * d;
      }
      se = wave_sum(se); q = wave_sum(q);
      if (W > 1) {
        if (lane == 0) { red[wave * 4] = se; red[wave * 4 + 1] = q; }
        __syncthreads();
        se = red[slot * W * 4]; q = red[slot * W * 4 + 1];
        for (int w = 1; w < W; ++w) { se += red[(slot * W + w) * 4]; q += red[(slot * W + w) * 4 + 1]; }
        __syncthreads();
      }
      if (live && sub == 0 && lane == 0) {
        if (a.lpd) a.lpd[i] = (mx + log(se)) - log((double)S);
        if (a.lmean) { a.lmean[i] = mean; a.lm2[i] = q; }
        if (wantPit) a.pit[i] = sp / (double)S;
      }
    }
  }
  if (a.Q == 0) return;

  __syncthreads();                                                                 // the row reductions are done with z
  for (int e = tid; e < N; e += QT_BLOCK) {
    const int r = e >> shift, j = e & (Sp - 1);
    if (j < S && row0 + r < a.chunkRows) {
      const uint64_t i = (uint64_t)(a.chunk0 + row0 + r);
      const double sd = a.sigma[j] * (a.rowScale ? a.rowScale[i] : 1.0);
      key[e] = qt_key(__longlong_as_double((long long)key[e]) + sd * philox_normal(a.key0, a.key1, i, (uint32_t)j));
    }
  }
  __syncthreads();
  qt_sort_rows(key, N, Sp);
  qt_type7_rows(a, key, row0);
}

// uploads, two launches per chunk of rows, the downloads — on `stream`, everything allocated here freed here (summary_run's discipline)
static void ppd_run(hipStream_t stream, int P, const PpdCall& c, int64_t& launches) {
  SummaryCall r = c.rows;
  const int link = r.link;
  r.link = 0;                                                     // k_predict_values writes z, whatever the response
  const ReadoutPlan plan = readout_plan(r, 0, 4, false);          // no reduction space; the workgroups are chosen per chunk
  const ChunkPlan cp = chunk_plan(r.nT, r.S, c.scratchBytes, QT_SCRATCH_DEFAULT, 1, 64);
  CallBuffers buf(stream);
  const size_t nT = (size_t)r.nT, S = (size_t)r.S, Q = (size_t)c.Q;
  const size_t rowLds = cp.sortLds + (size_t)8 * PP_RED;
  PpdDev a{};
  buf.upload_rows(a, r, P, plan.stageNodes);
  a.vals = buf.alloc<double>(nullptr, (size_t)cp.C * S);
  if (Q) { a.probs = buf.alloc(c.probs, Q); a.quantiles = buf.alloc<double>(nullptr, Q * nT); }
  if (!link) { a.sigma = buf.alloc(c.sigma, S); if (c.rowScale) a.rowScale = buf.alloc(c.rowScale, nT); }
  if (c.y) {
    a.y = buf.alloc(c.y, nT);
    if (c.lpd) a.lpd = buf.alloc<double>(nullptr, nT);
    if (c.lmean) { a.lmean = buf.alloc<double>(nullptr, nT); a.lm2 = buf.alloc<double>(nullptr, nT); }
    if (c.pit) a.pit = buf.alloc<double>(nullptr, nT);
  }
  a.key0 = (uint32_t)c.noiseKey; a.key1 = (uint32_t)(c.noiseKey >> 32); a.ppdLink = link;
  a.Q = c.Q; a.Sp = cp.Sp; a.R = cp.R;
  predict_values_prepare(plan);
  HIP_OK(hipFuncSetAttribute((const void*)k_ppd_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rowLds));
  LaunchCount launched{launches};
  for (int64_t ch = 0; ch < cp.chunks; ++ch) {
    a.chunk0 = ch * cp.C; a.chunkRows = std::min<int64_t>(cp.C, r.nT - a.chunk0);
    predict_values_launch(stream, plan, chunk_grid(a), a); launched();
    hipLaunchKernelGGL(k_ppd_rows, dim3((unsigned)((a.chunkRows + cp.R - 1) / cp.R)), dim3(QT_BLOCK), rowLds, stream, a); launched();
  }
  if (Q) HIP_OK(hipMemcpyAsync(c.quantiles, a.quantiles, Q * nT * 8, hipMemcpyDeviceToHost, stream));
  if (a.lpd) HIP_OK(hipMemcpyAsync(c.lpd, a.lpd, nT * 8, hipMemcpyDeviceToHost, stream));
  if (a.lmean) {
    HIP_OK(hipMemcpyAsync(c.lmean, a.lmean, nT * 8, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(c.lm2, a.lm2, nT * 8, hipMemcpyDeviceToHost, stream));
  }
  if (a.pit) HIP_OK(hipMemcpyAsync(c.pit, a.pit, nT * 8, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  r.info[0] = plan.staged ? 1 : 2; r.info[1] = cp.C; r.info[2] = cp.chunks; r.info[3] = ((int64_t)cp.R << 32) | (int64_t)cp.Sp;
  r.info[4] = r.maxDrawNodes; r.info[5] = launched.mine; r.info[6] = buf.bytes; r.info[7] = r.S;
}
