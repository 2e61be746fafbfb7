// Summaries of the stored-tree predictions, formed on the device WITHOUT the [rows x draws] matrix (s4b_predict_summary; DESIGN.md 5.5).
// Included by dev_hip.hip inside namespace s4b, in front of dev_pd.inc and dev_quantile.inc.  The walk, the staging, the linear part, the reduction and
// the route are dev_readout.inc's, which this file includes for all three.
//
// For row i and kept draw k
//     z(i,k) = bart(i,k) + offset[i] + sum_j dense[i,j] denseCoef[k,j] + sum_e ellValue[i,e] ellCoef[k, ellIndex[i,e]]      (ellIndex -1: skipped)
//     v(i,k) = z, or Phi(z) under link 1
// and the kernel returns, per row, the mean and the sum of squared deviations of v over the draws (Welford, in draw order, in the thread that owns
// the row) and, per draw, up to PS_GMAX sums of weights[g,i] * v over the rows.  Tiles: tile = blockIdx.x, += gridDim.x; every tile loops over all S
// draws.  Scratch of the per-draw sums: workgroups x S x G doubles.
// the tile geometry of the whole family stays in this file, where the GPU tests read it (tests/test_gpu_predict_summary.py, test_gpu_partial_dependence.py)
constexpr int PS_BLOCK = 1024;             // rows per tile = threads per workgroup (16 waves: four per SIMD share one staging)
constexpr int PS_STAGE_NODES = 3072;       // nodes per staging buffer at most (48 KB; two buffers)
constexpr int PS_WALK = 4;                 // trees walked at once per thread
#include "dev_readout.inc"

constexpr int PS_GMAX = 8;                 // weight vectors per call
constexpr size_t PS_RED_BYTES = (size_t)2 * PS_WAVES * PS_GMAX * 8;

struct SummaryDev : RowsDev { const double* weights; double* mean; double* m2; double* part; int G; };

template <bool STAGED>
__global__ __launch_bounds__(PS_BLOCK) void k_predict_summary(SummaryDev a) {
  extern __shared__ __align__(16) unsigned char ps_lds[];
  double* red = (double*)ps_lds;                                                   // [2][PS_WAVES][PS_GMAX]
  WalkNode* nbuf = (WalkNode*)(ps_lds + PS_RED_BYTES);                             // [2][stageNodes]
  int32_t* sbuf = (int32_t*)(ps_lds + PS_RED_BYTES + (size_t)2 * a.stageNodes * sizeof(WalkNode));   // [2][T]: tree starts inside the draw
  const int tid = threadIdx.x, T = a.T;
  const int64_t nT = a.nT, S = a.S;
  const int64_t tiles = (nT + PS_BLOCK - 1) / PS_BLOCK;

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i = tile * PS_BLOCK + tid;
    const bool act = i < nT;
    const size_t ii = (size_t)(act ? i : nT - 1);          // threads beyond the last row walk the last row with weight 0 and store nothing
    const double off = a.offset ? a.offset[ii] : 0.0;
    double mean = 0.0, m2 = 0.0;
    __syncthreads();                              // the tile before is done with both halves of `red` and with the staging buffers
    if (STAGED) { stage_draw<false>(a, 0, nbuf, sbuf, nullptr); __syncthreads(); }
    for (int64_t k = 0; k < S; ++k) {
      const int b = (int)(k & 1);
      // draw k + 1 into the other buffer (last read in draw k - 1, before that draw's barrier): a wave waits for its own few loads here while the
      // other waves walk draw k
      if (STAGED && k + 1 < S) stage_draw<false>(a, k + 1, nbuf + (size_t)(b ^ 1) * a.stageNodes, sbuf + (size_t)(b ^ 1) * T, nullptr);
      const double f = walk_all<STAGED>(a, nbuf + (size_t)b * a.stageNodes, sbuf + (size_t)b * T, k, ii);
      double z = response_scale(a, k, f);
      if (a.offset) z += off;
      z = add_linear(z, a, k, ii);
      const double v = a.link ? 0.5 * erfc(-z * 0.70710678118654752440) : z;
      const double d = v - mean;                  // Welford, in draw order
      mean += d / (double)(k + 1);
      m2 += d * (v - mean);
      // (the weights are read again per draw: registers go to the walk)
      for (int g = 0; g < a.G; ++g) red_store(red, PS_GMAX, b, g, act ? a.weights[(size_t)g * (size_t)nT + ii] * v : 0.0);
      __syncthreads();                            // draw k + 1 staged, the waves' sums of draw k visible, buffer b free
      red_fold(red, PS_GMAX, b, a.G, a.part, S, k, tile == (int64_t)blockIdx.x);
    }
    if (act) { a.mean[i] = mean; a.m2[i] = m2; }
  }
}

// uploads, the two launches, downloads — on `stream`, everything allocated here freed here (predict_stored's discipline)
static void summary_run(hipStream_t stream, int P, const SummaryCall& c, int64_t& launches) {
  const ReadoutPlan plan = readout_plan(c, PS_RED_BYTES, 4, true);
  CallBuffers buf(stream);
  const size_t nT = (size_t)c.nT, S = (size_t)c.S, G = (size_t)c.G;
  SummaryDev a{};
  buf.upload_rows(a, c, P, plan.stageNodes);
  double* average = nullptr;
  if (c.G) {
    a.weights = buf.alloc(c.weights, G * nT);
    a.part = buf.alloc<double>(nullptr, (size_t)plan.workgroups * S * G);
    average = buf.alloc<double>(nullptr, S * G);
  }
  a.mean = buf.alloc<double>(nullptr, nT); a.m2 = buf.alloc<double>(nullptr, nT);
  a.G = c.G;
  if (plan.staged) {
    HIP_OK(hipFuncSetAttribute((const void*)k_predict_summary<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
    hipLaunchKernelGGL(k_predict_summary<true>, dim3(plan.workgroups), dim3(PS_BLOCK), plan.lds, stream, a);
  } else hipLaunchKernelGGL(k_predict_summary<false>, dim3(plan.workgroups), dim3(PS_BLOCK), plan.lds, stream, a);
  HIP_OK(hipGetLastError()); ++launches; c.info[5] = 1;
  if (c.G) {
    fold_partials(stream, a.part, c.S * c.G, plan.workgroups, average, launches); c.info[5] = 2;
    HIP_OK(hipMemcpyAsync(c.average, average, S * G * 8, hipMemcpyDeviceToHost, stream));
  }
  HIP_OK(hipMemcpyAsync(c.mean, a.mean, nT * 8, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipMemcpyAsync(c.m2, a.m2, nT * 8, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  c.info[0] = plan.staged ? 1 : 2; c.info[1] = PS_BLOCK; c.info[2] = plan.workgroups; c.info[3] = (int64_t)plan.stageBytes;
  c.info[4] = c.maxDrawNodes; c.info[6] = buf.bytes; c.info[7] = plan.stageNodes;
}
