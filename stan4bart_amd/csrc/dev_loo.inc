// PSIS-LOO over the pooled kept draws (s4b_predict_loo; DESIGN.md 5.10): per row the Pareto-smoothed importance-sampling leave-one-out log predictive
// density, the Pareto shape khat of the importance ratios' tail, the lpd and the effective sample size of the weights, without the [rows x draws]
// matrix.  Included by dev_hip.hip inside namespace s4b, after dev_ppd.inc: the walk, the staging, the chunked value scratch and k_predict_values are
// dev_readout.inc's and dev_quantile.inc's, the LDS sort is dev_quantile.inc's, the log-likelihood is dev_ppd.inc's ppd_loglik.
//
// Per chunk of C rows two launches on the sampler's stream:
//   k_predict_values<STAGED>   UNCHANGED and always with link 0: the scratch holds z(i,k), predict_summary's z.
//   k_loo_rows                 a workgroup of QT_BLOCK threads owns R = max(1, 4096 / Sp) rows as k_ppd_rows does.  It loads its rows of z ONCE and
//                              overwrites every element with qt_key(-l(i,k)) — l is formed once per element —, then runs qt_sort_rows, unchanged:
//                              every row comes out as lr(0) <= ... <= lr(S-1), lr = -l the log importance ratio.
// THE SORTED ROW IS ENOUGH; no draw index travels through the sort.  With mx = lr(S-1) and lw(j) = lr(j) - mx the raw log weights, PSIS replaces the
// M largest by the quantiles of a generalised Pareto fitted to them, BY RANK: the j-th smallest of the tail gets the j-th quantile.  The estimate is
//     elpd_loo = log sum_j exp(lw'(j) + l(j)) - log sum_j exp(lw'(j)),   l(j) = -lr(j) the log-likelihood of the draw at sorted position j.
// Outside the tail lw'(j) + l(j) = (lr(j) - mx) - lr(j) = -mx whichever draw it is; inside the tail both operands are known by rank.  So every term
// is a function of the sorted position alone, and ties (equal lr at different draws) are harmless: the tied draws contribute equal l and receive
// weights whose sum does not depend on which of them gets which.  (Expectations of anything OTHER than the likelihood — LOO-PIT — would need the
// draw and its weight paired again: out of scope.)
//
// Per row, after the sort (a row belongs to W = max(1, 4 / R) waves, sub-wave `sub` of slot `slot`, as in k_ppd_rows; M = the tail length of the call):
//   A  no fit where M < 5 or lw(S-1) - lw(S-M) < 2^-52 / 100 (khat = +inf, raw weights).  Else ec = exp(lw(S-M-1)) and the W waves write
//      x(j) = exp(lw(S-M+j)) - ec, j < M ascending, into the row's M doubles behind the keys.
//   B  wave sub 0 fits the generalised Pareto (Zhang & Stephens 2009 as loo::gpdfit restates it): lane g - 1 owns grid point theta_g, G = 30 +
//      floor(sqrt M) <= 62 lanes; every lane runs over x(0 .. M-1) in ascending j (four partial sums, j mod 4), all lanes reading the same LDS address (a broadcast); max L,
//      sum w and sum theta w through wave_max / wave_sum; then k0 = mean_j log1p(-theta^ x(j)) lane-strided.  khat, sigma reach the row's other
//      waves through LDS.
//   C  the W waves overwrite x(j) by the smoothed lw'(S-M+j) = min(0, log(sigma expm1(-khat log1p(-p_j)) / khat + ec)), p_j = (j + 0.5) / M, and
//      take the maxima mB = max lw', mA = max(-mx, max_tail (lw' - lr)).
//   D  one pass over the sorted row: sB = sum exp(lw' - mB), sC = sum exp(lw' - mB)^2, sL = sum exp(lr(0) - lr(j)), and over the tail
//      sA = sum exp((lw' - lr) - mA); the S - M draws outside the tail add (S - M) exp(-mx - mA) to sA at the end.
//          elpd_loo = (mA + log sA) - (mB + log sB),  pareto_k = khat,  lpd = (-lr(0) + log sL) - log S,  ess = sB^2 / sC
// Every sum: lane-strided ascending, the xor butterfly, the W waves of a row folded in wave order through LDS between barriers the whole workgroup
// meets (the loops below are uniform over the workgroup).  No floating-point atomics: two calls return the same bits.
// LDS: 8 max(Sp, 4096) + 8 LOO_RED + 8 (4 / W) M bytes — keys, reduction space, the tails of the rows in flight; at S = 16384 with the largest
// admissible tail (1024): 128 KB + 256 B + 8 KB of the 160 KB of a compute unit.
constexpr int LOO_RED = 32;                // doubles of reduction space behind the keys: [4 waves][8] — 0, 1: khat, sigma; 2, 3: the maxima; 4 .. 7: the sums
constexpr int LOO_TAIL_MAX = 1024;         // the longest tail of a call: 8 KB of LDS per row in flight

struct LooDev : QuantileDev {
  const double* y; const double* sigma; const double* rowScale;          // [nT]; [S] (link 0); [nT] or NULL (= 1)
  double* elpd; double* khat; double* lpd; double* ess;                  // [nT] each, or NULL
  int looLink;                                                           // the response: 0 continuous, 1 binary.  RowsDev::link stays 0: the scratch holds z
  int M, G, quart;                                                       // tail length; grid points 30 + floor(sqrt M); floor(M / 4 + 0.5) - 1
};

__global__ __launch_bounds__(QT_BLOCK) void k_loo_rows(LooDev a) {
  extern __shared__ __align__(16) unsigned char lo_lds[];
  uint64_t* key = (uint64_t*)lo_lds;                                               // [R][Sp]: the keys of lr = -l
  const int tid = threadIdx.x, Sp = a.Sp, R = a.R, N = R * Sp, M = a.M;
  double* red = (double*)(lo_lds + (size_t)8 * N);                                 // [4][8]
  const int shift = 31 - __clz(Sp);                                                // Sp = 1 << shift
  const int S = (int)a.S;
  const int64_t row0 = (int64_t)blockIdx.x * R;                                    // first row of the workgroup inside the chunk
  const int link = a.looLink;
  for (int e = tid; e < N; e += QT_BLOCK) {
    const int r = e >> shift, j = e & (Sp - 1);
    uint64_t kk = ~0ull;
    if (j < S && row0 + r < a.chunkRows) {
      const size_t i = (size_t)(a.chunk0 + row0 + r);
      const double sd = link ? 1.0 : a.sigma[j] * (a.rowScale ? a.rowScale[i] : 1.0);
      double rr;
      kk = qt_key(-ppd_loglik(link, a.y[i], a.vals[(size_t)(row0 + r) * (size_t)S + (size_t)j], sd, rr));
    }
    key[e] = kk;
  }
  __syncthreads();
  qt_sort_rows(key, N, Sp);                                                        // (ends on a barrier)

  const int wave = tid >> 6, lane = tid & 63;
  const int W = R >= 4 ? 1 : 4 / R, slots = 4 / W;                                 // waves that share a row; rows in flight (R is a power of two)
  const int sub = wave % W, slot = wave / W, lead = slot * W;                      // lead: the first wave of the row
  double* xr = red + LOO_RED + (size_t)slot * M;                                   // [M]: first x, then the smoothed lw' of the tail
  for (int rb = 0; rb < R; rb += slots) {                                          // uniform over the workgroup: the barriers below are met by all
    const int r = rb + slot;
    const bool live = row0 + r < a.chunkRows;
    const size_t i = (size_t)(a.chunk0 + row0 + (live ? r : 0));
    const uint64_t* kr = key + (size_t)r * Sp;
    const double mx = qt_value(kr[S - 1]), lr0 = qt_value(kr[0]);
    // ---- A: is there a tail to fit?  x into LDS
    const bool fit = live && M >= 5 && mx - qt_value(kr[S - M]) >= 0x1p-52 / 100.0;          // (M <= S - 1: the host)
    const double ec = fit ? exp(qt_value(kr[S - M - 1]) - mx) : 0.0;
    if (fit) for (int j = sub * 64 + lane; j < M; j += 64 * W) xr[j] = exp(qt_value(kr[S - M + j]) - mx) - ec;
    __syncthreads();
    // ---- B: the generalised-Pareto fit, one wave
    double khat = INFINITY, sigma = 0.0;
    if (fit && sub == 0) {
      const double dM = (double)M;
      const bool on = lane < a.G;
      const double theta = 1.0 / xr[M - 1] + (1.0 - sqrt((double)a.G / ((double)lane + 0.5))) / (3.0 * xr[a.quart]);
      double kap = 0.0, kap1 = 0.0, kap2 = 0.0, kap3 = 0.0;                         // four partial sums: a quarter of the depth, four logarithms in flight
      int j4 = 0;
      for (; j4 + 3 < M; j4 += 4) {
        kap += log1p(-theta * xr[j4]); kap1 += log1p(-theta * xr[j4 + 1]); kap2 += log1p(-theta * xr[j4 + 2]); kap3 += log1p(-theta * xr[j4 + 3]);
      }
      for (; j4 < M; ++j4) kap += log1p(-theta * xr[j4]);
      kap = ((kap + kap1) + (kap2 + kap3)) / dM;
      const double L = on ? dM * (log(-theta / kap) - kap - 1.0) : -INFINITY;
      const double Lm = wave_max(L);
      const double w = on ? exp(L - Lm) : 0.0;
      const double sw = wave_sum(w), stw = wave_sum(on ? theta * w : 0.0);
      const double th = stw / sw;
      double k0 = 0.0;
      for (int j = lane; j < M; j += 64) k0 += log1p(-th * xr[j]);
      k0 = wave_sum(k0) / dM;
      sigma = -k0 / th;
      khat = k0 * dM / (dM + 10.0) + 5.0 / (dM + 10.0);
      if (!(fabs(khat) < INFINITY) || !(fabs(sigma) < INFINITY)) khat = INFINITY;          // not finite (a NaN included): no smoothing
      if (lane == 0) { red[wave * 8] = khat; red[wave * 8 + 1] = sigma; }
    }
    __syncthreads();
    if (fit) { khat = red[lead * 8]; sigma = red[lead * 8 + 1]; }
    const bool smooth = fit && khat < INFINITY;
    const int T0 = smooth ? S - M : S;                                             // the smoothed tail: sorted positions T0 .. S - 1
    // ---- C: the smoothed tail over x, the maxima
    double mB = smooth ? qt_value(kr[T0 - 1]) - mx : 0.0, mA = -mx;                // (the largest lw outside the tail; lw + l there)
    if (smooth) for (int j = sub * 64 + lane; j < M; j += 64 * W) {
      const double p = ((double)j + 0.5) / (double)M;
      const double v = fmin(0.0, log(sigma * expm1(-khat * log1p(-p)) / khat + ec));
      xr[j] = v;
      mB = fmax(mB, v); mA = fmax(mA, v - qt_value(kr[T0 + j]));
    }
    mB = wave_max(mB); mA = wave_max(mA);
    if (lane == 0) { red[wave * 8 + 2] = mB; red[wave * 8 + 3] = mA; }
    __syncthreads();
    for (int w = 0; w < W; ++w) { mB = fmax(mB, red[(lead + w) * 8 + 2]); mA = fmax(mA, red[(lead + w) * 8 + 3]); }
    // ---- D: the sums over the sorted row
    double sA = 0.0, sB = 0.0, sC = 0.0, sL = 0.0;
    if (live) for (int j = sub * 64 + lane; j < S; j += 64 * W) {
      const double lr = qt_value(kr[j]);
      const bool tail = j >= T0;
      double lw = lr - mx;
      if (tail) lw = xr[j - T0];
      const double t = exp(lw - mB);
      sB += t; sC += t * t; sL += exp(lr0 - lr);
      if (tail) sA += exp((lw - lr) - mA);
    }
    sA = wave_sum(sA); sB = wave_sum(sB); sC = wave_sum(sC); sL = wave_sum(sL);
    if (W > 1) {
      if (lane == 0) { red[wave * 8 + 4] = sA; red[wave * 8 + 5] = sB; red[wave * 8 + 6] = sC; red[wave * 8 + 7] = sL; }
      __syncthreads();
      sA = red[lead * 8 + 4]; sB = red[lead * 8 + 5]; sC = red[lead * 8 + 6]; sL = red[lead * 8 + 7];
      for (int w = 1; w < W; ++w) { sA += red[(lead + w) * 8 + 4]; sB += red[(lead + w) * 8 + 5]; sC += red[(lead + w) * 8 + 6]; sL += red[(lead + w) * 8 + 7]; }
    }
    if (live && sub == 0 && lane == 0) {
      sA += (double)T0 * exp(-mx - mA);
      if (a.elpd) a.elpd[i] = (mA + log(sA)) - (mB + log(sB));
      if (a.khat) a.khat[i] = khat;
      if (a.lpd) a.lpd[i] = (log(sL) - lr0) - log((double)S);
      if (a.ess) a.ess[i] = sB * sB / sC;
    }
    __syncthreads();                                                               // the row's tail and the reduction space are free again
  }
}

// uploads, two launches per chunk of rows, the downloads — on `stream`, everything allocated here freed here (summary_run's discipline)
static void loo_run(hipStream_t stream, int P, const LooCall& c, int64_t& launches) {
  SummaryCall r = c.rows;
  const int link = r.link;
  r.link = 0;                                                     // k_predict_values writes z, whatever the response
  const ReadoutPlan plan = readout_plan(r, 0, 4, false);          // no reduction space; the workgroups are chosen per chunk
  const ChunkPlan cp = chunk_plan(r.nT, r.S, c.scratchBytes, QT_SCRATCH_DEFAULT, 1, 64);
  CallBuffers buf(stream);
  const size_t nT = (size_t)r.nT, S = (size_t)r.S;
  const int slots = cp.R >= 4 ? 4 : cp.R;                         // rows in flight: 4 / W
  if (c.tailLen < 0 || c.tailLen > LOO_TAIL_MAX || (c.tailLen >= 5 && c.tailLen > r.S - 1)) throw std::logic_error("loo_run: tail length out of range");
  const size_t rowLds = cp.sortLds + (size_t)8 * LOO_RED + (size_t)8 * (size_t)slots * (size_t)c.tailLen;
  LooDev a{};
  buf.upload_rows(a, r, P, plan.stageNodes);
  a.vals = buf.alloc<double>(nullptr, (size_t)cp.C * S);
  if (!link) { a.sigma = buf.alloc(c.sigma, S); if (c.rowScale) a.rowScale = buf.alloc(c.rowScale, nT); }
  a.y = buf.alloc(c.y, nT);
  if (c.elpd) a.elpd = buf.alloc<double>(nullptr, nT);
  if (c.khat) a.khat = buf.alloc<double>(nullptr, nT);
  if (c.lpd) a.lpd = buf.alloc<double>(nullptr, nT);
  if (c.ess) a.ess = buf.alloc<double>(nullptr, nT);
  a.looLink = link; a.M = c.tailLen;
  int rt = 0; while ((rt + 1) * (rt + 1) <= a.M) ++rt;            // floor(sqrt M), in integers
  a.G = 30 + rt; a.quart = std::max(0, (2 * a.M + 4) / 8 - 1);    // floor(M / 4 + 0.5) - 1 = floor((2 M + 4) / 8) - 1
  a.Q = 0; a.Sp = cp.Sp; a.R = cp.R;
  predict_values_prepare(plan);
  HIP_OK(hipFuncSetAttribute((const void*)k_loo_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rowLds));
  LaunchCount launched{launches};
  for (int64_t ch = 0; ch < cp.chunks; ++ch) {
    a.chunk0 = ch * cp.C; a.chunkRows = std::min<int64_t>(cp.C, r.nT - a.chunk0);
    predict_values_launch(stream, plan, chunk_grid(a), a); launched();
    hipLaunchKernelGGL(k_loo_rows, dim3((unsigned)((a.chunkRows + cp.R - 1) / cp.R)), dim3(QT_BLOCK), rowLds, stream, a); launched();
  }
  if (a.elpd) HIP_OK(hipMemcpyAsync(c.elpd, a.elpd, nT * 8, hipMemcpyDeviceToHost, stream));
  if (a.khat) HIP_OK(hipMemcpyAsync(c.khat, a.khat, nT * 8, hipMemcpyDeviceToHost, stream));
  if (a.lpd) HIP_OK(hipMemcpyAsync(c.lpd, a.lpd, nT * 8, hipMemcpyDeviceToHost, stream));
  if (a.ess) HIP_OK(hipMemcpyAsync(c.ess, a.ess, nT * 8, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  r.info[0] = plan.staged ? 1 : 2; r.info[1] = cp.C; r.info[2] = cp.chunks; r.info[3] = ((int64_t)cp.R << 32) | (int64_t)cp.Sp;
  r.info[4] = r.maxDrawNodes; r.info[5] = launched.mine; r.info[6] = buf.bytes; r.info[7] = r.S;
}
