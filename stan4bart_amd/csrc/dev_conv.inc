// Split R-hat and effective sample size per row with the chains kept apart (s4b_predict_convergence; DESIGN.md 5.11): Stan's estimators over the
// pooled kept draws, without the [rows x draws] matrix, without a sort and without an FFT.
// Included by dev_hip.hip inside namespace s4b, after dev_loo.inc: the walk, the staging, the chunked value scratch and k_predict_values are
// dev_readout.inc's and dev_quantile.inc's, the log-likelihood is dev_ppd.inc's ppd_loglik.
//
// Per chunk of rows two launches on the sampler's stream:
//   k_predict_values<STAGED>   UNCHANGED: quantity 0 with the link as given (the scratch holds v), quantity 1 with link 0 (the scratch holds z).
//   k_chain_rows               a workgroup of QT_BLOCK threads owns R = max(1, 4096 / Sp) rows as k_loo_rows does and loads them ONCE into LDS as plain
//                              doubles (quantity 1: l(i,k), formed once per element).  A row belongs to W = max(1, 4 / R) waves.
// The host hands down C chain starts inside the pooled row and the common length N (the cut and the split are the host's: conv_chains).  A chain is
// N consecutive doubles of the row; what follows it in LDS need not belong to it, so every index is checked against N, never against the row.
//
// THE SUMMATION ORDER (the test model bounds it; nothing below depends on W, on which wave took which chain, or on the order the blocks are run in):
//   row maximum   quantity 1 only: max_k l over all S pooled draws (a maximum has no order), then x = exp(l - max) in place.
//   pass 1        chain c is taken by ONE wave (c mod W): sum_i x[i] lane-strided ascending (lane l: i = l, l + 64, ...), the xor butterfly
//                 (wave_sum), mu_c = sum / N — or the chain's value itself where min = max, so that a constant chain has q_c = 0 exactly —; d[i] = x[i] - mu_c stored in place; q_c = sum_i d[i]^2 likewise.  Then every wave of the row forms, over
//                 c lane-strided ascending and the butterfly: sum_c q_c, sum_c mu_c, mean = sum_c mu_c / C, sum_c (mu_c - mean)^2.
//   pass 2        lags in blocks of CV_LAGS = 64, lane l owns lag t = t0 + l.  A_c(t) = sum_{i < N - t} d_c[i] d_c[i + t] in four partial sums by
//                 i mod 4, each ascending in i, folded (p0 + p1) + (p2 + p3).  The chains are summed in FOUR groups by c mod 4, each ascending in c,
//                 through LDS: G(t) = (g0 + g1) + (g2 + g3) — group m is taken by wave m mod W, which changes nothing of the order.
//                 rho(t) = 1 - (W - G(t) / D) / var+, rho(0) = 1.  Pair sums P_j by one exchange with lane l ^ 1; the stopping rule by a ballot; the
//                 running minimum P'_j by an inclusive scan over the lanes carried from block to block; sum_{j < J} P'_j per block by the
//                 butterfly over the pairs below J (zeros elsewhere), the blocks added in ascending order.
// The number of blocks depends on the row.  The block loop is uniform over the workgroup all the same: a wave whose row has stopped (or has no row)
// goes on meeting the two barriers of a block until every wave of the workgroup reports that it has stopped.  It ends at t0 >= N at the latest.
// No floating-point atomics, no data-dependent order: two calls return the same bits.
// LDS: 8 max(Sp, 4096) + 8 CV_RED + 16 slots C + 8 slots 4 CV_LAGS bytes (slots = 4 / W rows in flight) — the rows, the reduction space, mu_c and
// q_c, the four group sums per lag; at S = 16384 and C = 256: 128 KB + 128 B + 4 KB + 2 KB of the 160 KB of a compute unit.
constexpr int CV_LAGS = 64;                // lags of a block: one per lane
constexpr int CV_RED = 16;                 // doubles of reduction space behind the rows: [4 waves] maxima, [4 waves] stop flags, 8 spare
constexpr int CV_CHAINS_MAX = 256;         // chains at most: 4 KB of LDS per row in flight

struct ConvDev : QuantileDev {
  const double* y; const double* sigma; const double* rowScale;          // quantity 1: [nT]; [S] (link 0); [nT] or NULL (= 1)
  const int32_t* chainStart;                                             // [C]: first draw of chain c inside the pooled row
  double* rhat; double* ess; double* mean; double* mcse; int32_t* nPairs;          // [nT] each, or NULL
  int quantity, convLink;                                                // convLink: the response of quantity 1 (RowsDev::link is 0 there)
  int C, N;                                                              // chains, their common length
};

__global__ __launch_bounds__(QT_BLOCK) void k_chain_rows(ConvDev a) {
  extern __shared__ __align__(16) unsigned char cv_lds[];
  double* xs = (double*)cv_lds;                                                    // [R][Sp]: x, then d
  const int tid = threadIdx.x, Sp = a.Sp, R = a.R, NE = R * Sp, C = a.C, N = a.N;
  const int wave = tid >> 6, lane = tid & 63;
  const int W = R >= 4 ? 1 : 4 / R, slots = 4 / W;                                 // waves that share a row; rows in flight (R is a power of two)
  const int sub = wave % W, slot = wave / W, lead = slot * W;
  double* red = xs + NE;                                                           // [CV_RED]
  double* mus = red + CV_RED + (size_t)slot * 2 * C;                               // [C] of this wave's row
  double* qs = mus + C;                                                            // [C]
  double* gs = red + CV_RED + (size_t)slots * 2 * C + (size_t)slot * 4 * CV_LAGS;  // [4][CV_LAGS] of this wave's row
  const int shift = 31 - __clz(Sp);                                                // Sp = 1 << shift
  const int S = (int)a.S, D = C * N;
  const int64_t row0 = (int64_t)blockIdx.x * R;                                    // first row of the workgroup inside the chunk
  const int link = a.convLink;
  for (int e = tid; e < NE; e += QT_BLOCK) {
    const int r = e >> shift, j = e & (Sp - 1);
    double v = 0.0;
    if (j < S && row0 + r < a.chunkRows) {
      v = a.vals[(size_t)(row0 + r) * (size_t)S + (size_t)j];
      if (a.quantity) {
        const size_t i = (size_t)(a.chunk0 + row0 + r);
        const double sd = link ? 1.0 : a.sigma[j] * (a.rowScale ? a.rowScale[i] : 1.0);
        double rr;
        v = ppd_loglik(link, a.y[i], v, sd, rr);
      }
    }
    xs[e] = v;
  }
  __syncthreads();

  const int jmax = N >= 4 ? (N - 4) / 2 : 0;                                       // the first j with 2 j + 1 >= N - 4
  const double dN = (double)N, dC = (double)C, dD = (double)D;
  for (int rb = 0; rb < R; rb += slots) {                                          // uniform over the workgroup: the barriers below are met by all
    const int r = rb + slot;
    const bool live = row0 + r < a.chunkRows;
    const size_t i = (size_t)(a.chunk0 + row0 + (live ? r : 0));
    double* xr = xs + (size_t)r * Sp;
    if (a.quantity) {                                                              // (uniform) ---- the likelihood up to a factor
      double mx = -INFINITY;
      if (live) for (int k = sub * 64 + lane; k < S; k += 64 * W) mx = fmax(mx, xr[k]);
      mx = wave_max(mx);
      if (lane == 0) red[wave] = mx;
      __syncthreads();
      for (int w = 0; w < W; ++w) mx = fmax(mx, red[lead + w]);
      if (live) for (int k = sub * 64 + lane; k < S; k += 64 * W) xr[k] = exp(xr[k] - mx);
      __syncthreads();
    }
    // ---- pass 1: the chain means, the centred series in place, the sums of squares
    if (live) for (int c = sub; c < C; c += W) {
      double* dc = xr + a.chainStart[c];
      double s = 0.0, lo = INFINITY, hi = -INFINITY;
      for (int k = lane; k < N; k += 64) { const double v = dc[k]; s += v; lo = fmin(lo, v); hi = fmax(hi, v); }
      lo = wave_min(lo); hi = wave_max(hi); s = wave_sum(s);
      const double mu = lo == hi ? lo : s / dN;                          // a constant chain: its value itself, so d = 0 and q_c = 0 EXACTLY
      double q = 0.0;
      for (int k = lane; k < N; k += 64) { const double d = dc[k] - mu; dc[k] = d; q += d * d; }
      q = wave_sum(q);
      if (lane == 0) { mus[c] = mu; qs[c] = q; }
    }
    __syncthreads();
    double sq = 0.0, sm = 0.0, sb = 0.0;
    if (live) {
      for (int c = lane; c < C; c += 64) { sq += qs[c]; sm += mus[c]; }
      sq = wave_sum(sq); sm = wave_sum(sm);
    }
    const double mean = sm / dC;
    if (live) {
      for (int c = lane; c < C; c += 64) { const double e = mus[c] - mean; sb += e * e; }
      sb = wave_sum(sb);
    }
    const double Wv = sq / (double)((N - 1) * C);
    const double vp = Wv * (double)(N - 1) / dN + (C > 1 ? sb / (double)(C - 1) : 0.0);
    const bool ok = live && N >= 4 && Wv > 0.0 && vp < INFINITY;                  // (a value that is not finite leaves W or var+ not finite)
    // ---- pass 2: blocks of lags until the pair sequence stops
    bool done = !ok;
    int J = 0;
    double sumP = 0.0, carry = INFINITY, eJ = 1.0, PJ = 0.0;
    for (int t0 = 0; t0 < N; t0 += CV_LAGS) {                                      // uniform: left together, below
      const int t = t0 + lane, n = N - t;                                          // lane's lag; its terms i = 0 .. n - 1 (none where n <= 0)
      if (!done) for (int m = sub; m < 4; m += W) {
        double g = 0.0;
        for (int c = m; c < C; c += 4) {
          const double* dc = xr + a.chainStart[c];
          double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
          int k = 0;
          for (; k + 3 < n; k += 4) {                                              // dc[k]: one address for the wave; dc[k + t]: consecutive lanes
            p0 += dc[k] * dc[k + t]; p1 += dc[k + 1] * dc[k + 1 + t]; p2 += dc[k + 2] * dc[k + 2 + t]; p3 += dc[k + 3] * dc[k + 3 + t];
          }
          if (k < n) p0 += dc[k] * dc[k + t];
          if (k + 1 < n) p1 += dc[k + 1] * dc[k + 1 + t];
          if (k + 2 < n) p2 += dc[k + 2] * dc[k + 2 + t];
          g += (p0 + p1) + (p2 + p3);
        }
        gs[m * CV_LAGS + lane] = g;
      }
      __syncthreads();
      if (!done) {
        const double G = (gs[lane] + gs[CV_LAGS + lane]) + (gs[2 * CV_LAGS + lane] + gs[3 * CV_LAGS + lane]);
        const double rho = t == 0 ? 1.0 : 1.0 - (Wv - G / dD) / vp;
        const double oth = wave_xor<1>(rho);
        const double P = rho + oth, ev = (lane & 1) ? oth : rho;                   // the pair's sum and its even entry, in both lanes of the pair
        const int j = t >> 1;
        const unsigned long long stop = __ballot(!(P > 0.0) || j >= jmax);
        double pm = P;                                                             // inclusive running minimum over the lanes (a pair holds it twice)
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const double up = __shfl_up(pm, o); if (lane >= o) pm = fmin(pm, up); }
        pm = fmin(pm, carry);
        const int first = stop ? __ffsll((long long)stop) - 1 : 64;                // the even lane of pair J, where it is in this block
        sumP += wave_sum((lane & 1) == 0 && lane < first ? pm : 0.0);
        if (stop) { J = (t0 + first) >> 1; eJ = __shfl(ev, first); PJ = __shfl(P, first); done = true; }
        else carry = __shfl(pm, 63);
      }
      if (lane == 0) red[4 + wave] = done ? 1.0 : 0.0;
      __syncthreads();
      if (red[4] + red[5] + red[6] + red[7] == 4.0) break;                         // every wave of the workgroup has stopped
    }
    if (live && sub == 0 && lane == 0) {
      double rhat = NAN, ess = NAN, mcse = NAN;
      if (ok) {
        const double eSt = J == 0 ? 1.0 : (PJ >= 0.0 ? eJ : 0.0);
        const double tau = -1.0 + 2.0 * (sumP + eSt) + (eJ > 0.0 ? eJ : 0.0);
        ess = fmin(dD / tau, dD * log10(dD));
        mcse = sqrt((sq + dN * sb) / (double)(D - 1)) / sqrt(ess);
        if (C > 1) rhat = sqrt(vp / Wv);
      }
      if (a.rhat) a.rhat[i] = rhat;
      if (a.ess) a.ess[i] = ess;
      if (a.mean) a.mean[i] = ok ? mean : NAN;
      if (a.mcse) a.mcse[i] = mcse;
      if (a.nPairs) a.nPairs[i] = ok ? J : -1;
    }
    __syncthreads();                                                               // the reduction space is free again
  }
}

// uploads, two launches per chunk of rows, the downloads — on `stream`, everything allocated here freed here (summary_run's discipline)
static void conv_run(hipStream_t stream, int P, const ConvCall& c, int64_t& launches) {
  SummaryCall r = c.rows;
  const int link = r.link;
  if (c.quantity) r.link = 0;                                     // k_predict_values writes z, whatever the response
  const ReadoutPlan plan = readout_plan(r, 0, 4, false);          // no reduction space; the workgroups are chosen per chunk
  const ChunkPlan cp = chunk_plan(r.nT, r.S, c.scratchBytes, QT_SCRATCH_DEFAULT, 1, 64);
  CallBuffers buf(stream);
  const size_t nT = (size_t)r.nT, S = (size_t)r.S;
  const int slots = cp.R >= 4 ? 4 : cp.R;                         // rows in flight: 4 / W
  if (c.numChains < 1 || c.numChains > CV_CHAINS_MAX || c.chainLen < 1) throw std::logic_error("conv_run: chains out of range");
  for (int x = 0; x < c.numChains; ++x)
    if (c.chainStart[x] < 0 || (int64_t)c.chainStart[x] + c.chainLen > r.S) throw std::logic_error("conv_run: a chain leaves the pooled row");
  const size_t rowLds = cp.sortLds + (size_t)8 * CV_RED + (size_t)16 * (size_t)slots * (size_t)c.numChains + (size_t)8 * (size_t)slots * 4 * CV_LAGS;
  ConvDev a{};
  buf.upload_rows(a, r, P, plan.stageNodes);
  a.vals = buf.alloc<double>(nullptr, (size_t)cp.C * S);
  if (c.quantity) {
    if (!link) { a.sigma = buf.alloc(c.sigma, S); if (c.rowScale) a.rowScale = buf.alloc(c.rowScale, nT); }
    a.y = buf.alloc(c.y, nT);
  }
  a.chainStart = buf.alloc(c.chainStart, (size_t)c.numChains);
  if (c.rhat) a.rhat = buf.alloc<double>(nullptr, nT);
  if (c.ess) a.ess = buf.alloc<double>(nullptr, nT);
  if (c.mean) a.mean = buf.alloc<double>(nullptr, nT);
  if (c.mcse) a.mcse = buf.alloc<double>(nullptr, nT);
  if (c.nPairs) a.nPairs = buf.alloc<int32_t>(nullptr, nT);
  a.quantity = c.quantity; a.convLink = link; a.C = c.numChains; a.N = c.chainLen;
  a.Q = 0; a.Sp = cp.Sp; a.R = cp.R;
  predict_values_prepare(plan);
  HIP_OK(hipFuncSetAttribute((const void*)k_chain_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rowLds));
  LaunchCount launched{launches};
  for (int64_t ch = 0; ch < cp.chunks; ++ch) {
    a.chunk0 = ch * cp.C; a.chunkRows = std::min<int64_t>(cp.C, r.nT - a.chunk0);
    predict_values_launch(stream, plan, chunk_grid(a), a); launched();
    hipLaunchKernelGGL(k_chain_rows, dim3((unsigned)((a.chunkRows + cp.R - 1) / cp.R)), dim3(QT_BLOCK), rowLds, stream, a); launched();
  }
  if (a.rhat) HIP_OK(hipMemcpyAsync(c.rhat, a.rhat, nT * 8, hipMemcpyDeviceToHost, stream));
  if (a.ess) HIP_OK(hipMemcpyAsync(c.ess, a.ess, nT * 8, hipMemcpyDeviceToHost, stream));
  if (a.mean) HIP_OK(hipMemcpyAsync(c.mean, a.mean, nT * 8, hipMemcpyDeviceToHost, stream));
  if (a.mcse) HIP_OK(hipMemcpyAsync(c.mcse, a.mcse, nT * 8, hipMemcpyDeviceToHost, stream));
  if (a.nPairs) HIP_OK(hipMemcpyAsync(c.nPairs, a.nPairs, nT * 4, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  r.info[0] = plan.staged ? 1 : 2; r.info[1] = cp.C; r.info[2] = cp.chunks; r.info[3] = ((int64_t)cp.R << 32) | (int64_t)cp.Sp;
  r.info[4] = r.maxDrawNodes; r.info[5] = launched.mine; r.info[6] = buf.bytes; r.info[7] = r.S;
}
