// Order statistics ACROSS THE ROWS within one pooled draw, summarised over the draws, and who lies beyond them (s4b_predict_sorted; DESIGN.md 5.18):
// for rows i < n and pooled draws k < S let y_k(0) <= ... <= y_k(n-1) be the column x(., k) in the order of qt_key (-0.0 before +0.0),
//     x = k_predict_values' v (one arm) or k_contrast_values' d (two arms).
//     sorted[j, k] = R's type 7 across the rows at row_probs[j]: h = p (n - 1), lo = floor(h), hi = min(lo + 1, n - 1), g = h - lo, formed on the host as
//                    qt_type7_rows forms them; y(lo) where g = 0, else y(lo) + g (y(hi) - y(lo)),
//     cut[c, k]    = y_k(cut_rank[c]), the order statistic itself,
//     n_above[c, i] = #{k : x(i,k) > cut[c,k]},  n_below[c, i] = #{k : x(i,k) < cut[c,k]}, strict, in double comparison,
// the matrix D [(Qr + J) x S] of the sorted and the cut rows, and per statistic the mean, m2 and type-7 quantiles over the draws.
// Included by dev_hip.hip inside namespace s4b, after readout_describe.inc: the value kernels, the monotone key, the call scaffold and the summary over
// the draws (k_level_rows, k_row_quantiles, unchanged) are dev_readout.inc's, dev_quantile.inc's, dev_contrast.inc's and dev_groups.inc's.  New here is
// the selection of order statistics across the rows, which no sum over the rows can form.
//
// BLOCKS OF DRAWS.  The other chunked read-outs hold a chunk of rows with all draws; a statistic across the rows needs all rows of a block of draws.
// Every per-draw array of RowsDev / ContrastDev is addressed as base + k * stride (treeStart, scale, denseCoef, ellCoef, order, numBase), and the tree
// starts are absolute node indices.  So the block [kb, kb + Db) is a VIEW: a copy of the device struct with those pointers advanced by kb, S = Db,
// numNodes = the first node of draw kb + Db (stage_draw reads numNodes for the last draw of a view), chunk0 = 0 and chunkRows = n.  The value kernels
// run unchanged on it and write vals[i Db + k'] for all rows: the trees are walked ONCE per (row, draw), never once per selection pass.
//
// THE SELECTION, a radix select over qt_key, 8 passes of 8-bit digits from the most significant.  The targets of a draw are the distinct ranks among the
// lo and hi ranks of the row probs and the cut ranks, ascending, U <= SO_TARGETS_MAX.  A target's state is a prefix (the digits found so far) and the
// rank that remains inside the keys that share the prefix.  Order statistics are monotone in the rank, so in ascending rank order the prefixes never
// decrease: targets with the same prefix are neighbours, and the distinct prefixes of a draw ("nodes") are sorted without a sort.
//   k_sorted_hist<DPW>   grid: row workgroups x groups of DPW draws.  A thread reads its row's DPW draws (DPW = 8: one whole 64-byte segment), finds the
//                        node whose prefix its key carries by a binary search among the draw's nodes staged in LDS (no node: the key is out of
//                        play), and counts the next digit in the node's table of 256 uint32 in LDS, 1 KiB per (draw, node), by integer atomicAdd.
//                        The lanes of a wave work on the same draw at once; where all of them that count agree on (node, digit) — the first passes
//                        of nearly every column: same sign, same exponent — one lane adds the popcount.  The tables go to global memory by integer
//                        atomicAdd of the non-zero counts.  DPW is chosen so that the tables take 64 KiB at most: two workgroups per compute unit.
//   k_sorted_scan        a workgroup per draw, a wave per target in turn: the 256 counts of the target's node, four per lane, a wave prefix sum, the
//                        digit at which the running count passes the remaining rank; then the tables just read are zeroed for the next pass and one
//                        thread forms the next list of nodes from the neighbours.  The last pass stores the key of the order statistic and puts the
//                        state back to the start for the next block.
//   k_sorted_count       a thread per row: its Db values against the block's cuts staged in LDS, counted in registers, stored by the owning thread
//                        (the first block stores, later ones add: the blocks follow each other on the stream).
//   k_sorted_finish      after the last block: the interpolation into D.
// Integer sums only: the result is a function of the columns' multisets, whatever the grid, the block of draws, the route or the order of the adds.
// No floating-point atomics.  Device memory beyond the value kernel's: vals 8 n Db, the tables 1 KiB x U x Db (at most 32 MiB), the order statistics
// 8 U S, the counts 8 J n, D and the summaries.
constexpr int SO_BLOCK = 256;                    // threads per workgroup of the four kernels
constexpr int SO_TARGETS_MAX = 32;               // distinct ranks per draw at most: 2 S4B_SORTED_PROBS_MAX + S4B_SORTED_CUTS_MAX
constexpr int SO_PROBS_MAX = 12;                 // S4B_SORTED_PROBS_MAX
constexpr int SO_CUTS_MAX = 8;                   // S4B_SORTED_CUTS_MAX
constexpr int SO_PASSES = 8;                     // 8-bit digits of a 64-bit key
constexpr int SO_DRAWS_MAX = 1024;               // draws per block at most: bounds the tables in global memory to 32 MiB
constexpr size_t SO_TABLE_LDS = 64 * 1024;       // the LDS tables of a workgroup of k_sorted_hist at most
constexpr int SO_HIST_GRID = 1024;               // workgroups of k_sorted_hist, about
constexpr int SO_HIST_TILES = 4;                 // tiles of SO_BLOCK rows a workgroup of k_sorted_hist takes at least where there are that many: the flush is paid once
#ifndef S4B_SO_SCRATCH_MIB
#define S4B_SO_SCRATCH_MIB 64                    // the value scratch of a block of draws (DESIGN.md 5.18); a measurement build may set another (tools/sorted_probe.py)
#endif
constexpr int64_t SO_SCRATCH_DEFAULT = (int64_t)S4B_SO_SCRATCH_MIB << 20;

struct SortedDev {
  const double* vals; int64_t n, stride;         // the block's values vals[i stride + k'], k' < Db
  int Db, U, J, L, pass, aligned, first;         // draws of the block, targets, cuts, statistics; aligned: 16-byte loads of a row's group are in place
  int64_t S, kb;                                 // all draws, the block's first draw
  uint64_t* prefix; uint32_t* rem; int32_t* node;          // [Db x U] per target: the digits so far, the rank that remains, its node
  uint64_t* nodePrefix; int32_t* nNodes;                   // [Db x U] ascending distinct prefixes, [Db]
  uint32_t* hist;                                          // [Db x U x 256] per (draw, node): zero between the passes
  uint64_t* ostat;                                         // [U x S] keys of the order statistics
  int32_t* nAbove; int32_t* nBelow;                        // [J x n] each, or NULL
  double* out;                                             // D [L x S]
  int32_t rank[SO_TARGETS_MAX];                            // the targets, ascending and distinct
  int32_t cutTarget[SO_CUTS_MAX];                          // the target of every cut
  int32_t statLo[SO_TARGETS_MAX], statHi[SO_TARGETS_MAX]; double statG[SO_TARGETS_MAX];          // per row of D: the targets of lo and hi, and g
};

// one count into the LDS tables for every lane of the wave (idx < 0: none): where the counting lanes agree, their first adds the popcount
__device__ __forceinline__ void so_add(uint32_t* tab, int idx) {
  const unsigned long long valid = __ballot(idx >= 0);
  if (!valid) return;
  const int leader = __ffsll((long long)valid) - 1;
  const int lead = __shfl(idx, leader);
  const unsigned long long same = __ballot(idx == lead);
  if (same == valid) { if ((int)(threadIdx.x & 63) == leader) atomicAdd(&tab[lead], (uint32_t)__popcll(valid)); }
  else if (idx >= 0) atomicAdd(&tab[idx], 1u);
}

template <int DPW>
__global__ __launch_bounds__(SO_BLOCK) void k_sorted_hist(SortedDev a) {
  extern __shared__ __align__(16) unsigned char so_lds[];
  const int tid = threadIdx.x, U = a.U, pass = a.pass;
  uint32_t* tab = (uint32_t*)so_lds;                                               // [DPW][U][256]
  uint64_t* np = (uint64_t*)(tab + (size_t)DPW * U * 256);                         // [DPW][U]: the nodes' prefixes, ascending
  int32_t* nn = (int32_t*)(np + (size_t)DPW * U);                                  // [DPW]
  const int k0 = (int)blockIdx.y * DPW, nd = min(DPW, a.Db - k0);                  // the group's first draw inside the block, its draws
  for (int e = tid; e < DPW * U * 256; e += SO_BLOCK) tab[e] = 0u;
  for (int e = tid; e < nd * U; e += SO_BLOCK) np[e] = a.nodePrefix[(size_t)k0 * U + e];
  if (tid < DPW) nn[tid] = tid < nd ? a.nNodes[k0 + tid] : 0;
  __syncthreads();
  const int shiftP = 64 - 8 * pass, shiftD = 56 - 8 * pass;
  const int64_t n = a.n, tiles = (n + SO_BLOCK - 1) / SO_BLOCK;
  const bool wide = a.aligned && nd == DPW && DPW >= 2;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i = tile * SO_BLOCK + tid;
    const bool act = i < n;
    const double* v = a.vals + (size_t)(act ? i : n - 1) * (size_t)a.stride + (size_t)k0;
    double x[DPW];
    if (wide) {
#pragma unroll
      for (int u = 0; u < DPW / 2; ++u) { const double2 p = ((const double2*)v)[u]; x[2 * u] = p.x; x[2 * u + 1] = p.y; }
    } else {
#pragma unroll
      for (int u = 0; u < DPW; ++u) x[u] = u < nd ? v[u] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < DPW; ++u) {
      int idx = -1;
      if (act && u < nd) {
        const uint64_t key = qt_key(x[u]), p = pass ? key >> shiftP : 0ull;
        const uint64_t* q = np + u * U;
        int lo = 0, hi = nn[u];                                                    // the first node whose prefix is not below p
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (q[mid] < p) lo = mid + 1; else hi = mid; }
        if (lo < nn[u] && q[lo] == p) idx = (u * U + lo) * 256 + (int)((key >> shiftD) & 255);
      }
      so_add(tab, idx);
    }
  }
  __syncthreads();
  uint32_t* dst = a.hist + (size_t)k0 * U * 256;                                   // (the same layout as the tables)
  for (int e = tid; e < nd * U * 256; e += SO_BLOCK) { const uint32_t c = tab[e]; if (c) atomicAdd(&dst[e], c); }
}

__global__ __launch_bounds__(SO_BLOCK) void k_sorted_scan(SortedDev a) {
  extern __shared__ __align__(16) unsigned char so_lds[];
  uint64_t* newp = (uint64_t*)so_lds;                                              // [U]
  uint32_t* newr = (uint32_t*)(newp + SO_TARGETS_MAX);                             // [U]
  const int tid = threadIdx.x, lane = tid & 63, U = a.U, d = blockIdx.x;
  const int nn = a.nNodes[d];
  for (int t = tid >> 6; t < U; t += SO_BLOCK / 64) {
    const int nd = a.node[d * U + t];
    const uint4 c = ((const uint4*)(a.hist + ((size_t)d * U + nd) * 256))[lane];   // bins 4 lane .. 4 lane + 3
    const uint32_t s = c.x + c.y + c.z + c.w, r = a.rem[d * U + t];
    uint32_t inc = s;                                                              // the running count up to and with this lane's bins
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t up = (uint32_t)__shfl_up((int)inc, o); if (lane >= o) inc += up; }
    const unsigned long long past = __ballot(inc > r);
    const int at = past ? __ffsll((long long)past) - 1 : 63;                       // (a rank below the node's count: some lane passes it)
    if (lane == at) {
      uint32_t rr = r - (inc - s);
      int g = 0;
      if (rr >= c.x) { rr -= c.x; g = 1; if (rr >= c.y) { rr -= c.y; g = 2; if (rr >= c.z) { rr -= c.z; g = 3; } } }
      newp[t] = (a.prefix[d * U + t] << 8) | (uint64_t)(4 * at + g);
      newr[t] = rr;
    }
  }
  __syncthreads();
  uint32_t* h = a.hist + (size_t)d * U * 256;
  for (int e = tid; e < nn * 256; e += SO_BLOCK) h[e] = 0u;                        // the tables this pass filled: the draw's first nn
  if (tid == 0) {
    const bool last = a.pass == SO_PASSES - 1;
    int cnt = 0;
    for (int t = 0; t < U; ++t) {
      const uint64_t p = newp[t];
      if (last) {                                                                  // the key itself; the state of the next block's first pass
        a.ostat[(size_t)t * (size_t)a.S + (size_t)(a.kb + d)] = p;
        a.prefix[d * U + t] = 0ull; a.rem[d * U + t] = (uint32_t)a.rank[t]; a.node[d * U + t] = 0;
      } else {
        if (t == 0 || p != newp[t - 1]) a.nodePrefix[d * U + cnt++] = p;           // ascending ranks: equal prefixes are neighbours
        a.prefix[d * U + t] = p; a.rem[d * U + t] = newr[t]; a.node[d * U + t] = cnt - 1;
      }
    }
    if (last) { a.nodePrefix[d * U] = 0ull; cnt = 1; }
    a.nNodes[d] = cnt;
  }
}

__global__ __launch_bounds__(SO_BLOCK) void k_sorted_count(SortedDev a) {
  extern __shared__ __align__(16) unsigned char so_lds[];
  double* cut = (double*)so_lds;                                                   // [J][Db]
  const int tid = threadIdx.x, J = a.J, Db = a.Db;
  for (int e = tid; e < J * Db; e += SO_BLOCK) {
    const int c = e / Db, k = e - c * Db;
    cut[e] = qt_value(a.ostat[(size_t)a.cutTarget[c] * (size_t)a.S + (size_t)(a.kb + k)]);
  }
  __syncthreads();
  const int64_t n = a.n, tiles = (n + SO_BLOCK - 1) / SO_BLOCK;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i = tile * SO_BLOCK + tid;
    if (i >= n) continue;
    const double* v = a.vals + (size_t)i * (size_t)a.stride;
    int ab[SO_CUTS_MAX], bl[SO_CUTS_MAX];
#pragma unroll
    for (int c = 0; c < SO_CUTS_MAX; ++c) { ab[c] = 0; bl[c] = 0; }
#pragma unroll 8
    for (int k = 0; k < Db; ++k) {
      const double x = v[k];
#pragma unroll
      for (int c = 0; c < SO_CUTS_MAX; ++c)
        if (c < J) { const double t = cut[c * Db + k]; ab[c] += x > t ? 1 : 0; bl[c] += x < t ? 1 : 0; }          // (the cut: the same LDS word for every lane)
    }
#pragma unroll
    for (int c = 0; c < SO_CUTS_MAX; ++c)
      if (c < J) {
        const size_t e = (size_t)c * (size_t)n + (size_t)i;
        if (a.nAbove) a.nAbove[e] = a.first ? ab[c] : a.nAbove[e] + ab[c];
        if (a.nBelow) a.nBelow[e] = a.first ? bl[c] : a.nBelow[e] + bl[c];
      }
  }
}

__global__ __launch_bounds__(SO_BLOCK) void k_sorted_finish(SortedDev a) {
  const int64_t S = a.S, m = (int64_t)a.L * S;
  for (int64_t x = (int64_t)blockIdx.x * SO_BLOCK + threadIdx.x; x < m; x += (int64_t)gridDim.x * SO_BLOCK) {
    const int j = (int)(x / S);
    const int64_t k = x - (int64_t)j * S;
    const double g = a.statG[j];
    const double xl = qt_value(a.ostat[(size_t)a.statLo[j] * (size_t)S + (size_t)k]);
    const double xh = qt_value(a.ostat[(size_t)a.statHi[j] * (size_t)S + (size_t)k]);
    a.out[x] = g == 0.0 ? xl : xl + g * (xh - xl);
  }
}

// the targets of a call: the ranks the statistics need (per statistic lo, hi and g) and the cuts, as the ascending distinct ranks and the indices into them
static void sorted_targets(SortedDev& d, int L, const int64_t* lo, const int64_t* hi, const double* g, int J, const int32_t* cutRank) {
  std::vector<int64_t> all;
  for (int j = 0; j < L; ++j) { all.push_back(lo[j]); all.push_back(hi[j]); }
  for (int c = 0; c < J; ++c) all.push_back(cutRank[c]);
  std::sort(all.begin(), all.end());
  all.erase(std::unique(all.begin(), all.end()), all.end());
  if ((int)all.size() > SO_TARGETS_MAX) throw std::invalid_argument("sorted: more than " + std::to_string(SO_TARGETS_MAX) + " distinct ranks per draw");
  auto at = [&](int64_t rank) { return (int32_t)(std::lower_bound(all.begin(), all.end(), rank) - all.begin()); };
  d.U = (int)all.size(); d.L = L; d.J = J;
  for (int t = 0; t < d.U; ++t) d.rank[t] = (int32_t)all[t];
  for (int j = 0; j < L; ++j) { d.statLo[j] = at(lo[j]); d.statHi[j] = at(hi[j]); d.statG[j] = g[j]; }
  for (int c = 0; c < J; ++c) d.cutTarget[c] = at(cutRank[c]);
}
// draws per workgroup of k_sorted_hist: the LDS tables within SO_TABLE_LDS
static int sorted_group(int U) { return U <= 8 ? 8 : U <= 16 ? 4 : 2; }
static size_t sorted_hist_lds(int dpw, int U) { return (size_t)dpw * U * 1024 + (size_t)dpw * U * 8 + (size_t)dpw * 4; }
// the state of the selection for blocks of at most Db draws, at the start of a block's first pass; once per call
static void sorted_state(CallBuffers& buf, SortedDev& d, int64_t Db, int64_t S, int64_t n) {
  const size_t U = (size_t)d.U, m = (size_t)Db * U;
  std::vector<uint32_t> rem(m);
  std::vector<int32_t> ones((size_t)Db, 1);
  for (size_t e = 0; e < m; ++e) rem[e] = (uint32_t)d.rank[e % U];
  d.prefix = buf.alloc<uint64_t>(nullptr, m); d.nodePrefix = buf.alloc<uint64_t>(nullptr, m); d.node = buf.alloc<int32_t>(nullptr, m);
  d.hist = buf.alloc<uint32_t>(nullptr, m * 256);
  HIP_OK(hipMemsetAsync(d.prefix, 0, m * 8, buf.stream)); HIP_OK(hipMemsetAsync(d.nodePrefix, 0, m * 8, buf.stream));
  HIP_OK(hipMemsetAsync(d.node, 0, m * 4, buf.stream)); HIP_OK(hipMemsetAsync(d.hist, 0, m * 1024, buf.stream));
  d.rem = buf.alloc(rem.data(), m); d.nNodes = buf.alloc(ones.data(), (size_t)Db);
  HIP_OK(hipStreamSynchronize(buf.stream));                                        // (rem and ones leave the scope)
  d.ostat = buf.alloc<uint64_t>(nullptr, U * (size_t)S);
  d.S = S; d.n = n;
  const int dpw = sorted_group(d.U);
  const int lds = (int)sorted_hist_lds(dpw, d.U);
  if (dpw == 8) HIP_OK(hipFuncSetAttribute((const void*)k_sorted_hist<8>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  else if (dpw == 4) HIP_OK(hipFuncSetAttribute((const void*)k_sorted_hist<4>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  else HIP_OK(hipFuncSetAttribute((const void*)k_sorted_hist<2>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  HIP_OK(hipFuncSetAttribute((const void*)k_sorted_count, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)SO_CUTS_MAX * SO_DRAWS_MAX * 8)));
}
// one block of draws [kb, kb + Db) whose values are at vals[i stride + k']: the 8 passes, then the counts where there are cuts and an output for them
static void sorted_block(hipStream_t stream, LaunchCount& launched, SortedDev& d, const double* vals, int64_t stride, int64_t kb, int Db) {
  d.vals = vals; d.stride = stride; d.kb = kb; d.Db = Db; d.first = kb == 0;
  d.aligned = ((uintptr_t)vals % 16 == 0) && (stride % 2 == 0);
  const int dpw = sorted_group(d.U);
  const size_t lds = sorted_hist_lds(dpw, d.U);
  const int64_t tiles = (d.n + SO_BLOCK - 1) / SO_BLOCK;
  const unsigned gy = (unsigned)((Db + dpw - 1) / dpw);
  const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((tiles + SO_HIST_TILES - 1) / SO_HIST_TILES, std::max<int64_t>(1, SO_HIST_GRID / gy)));
  for (int pass = 0; pass < SO_PASSES; ++pass) {
    d.pass = pass;
    if (dpw == 8) hipLaunchKernelGGL(k_sorted_hist<8>, dim3(gx, gy), dim3(SO_BLOCK), lds, stream, d);
    else if (dpw == 4) hipLaunchKernelGGL(k_sorted_hist<4>, dim3(gx, gy), dim3(SO_BLOCK), lds, stream, d);
    else hipLaunchKernelGGL(k_sorted_hist<2>, dim3(gx, gy), dim3(SO_BLOCK), lds, stream, d);
    launched();
    hipLaunchKernelGGL(k_sorted_scan, dim3((unsigned)Db), dim3(SO_BLOCK), (size_t)SO_TARGETS_MAX * 12, stream, d); launched();
  }
  if (d.J && (d.nAbove || d.nBelow)) {
    hipLaunchKernelGGL(k_sorted_count, dim3((unsigned)std::min<int64_t>(tiles, GRID_MAX)), dim3(SO_BLOCK), (size_t)d.J * (size_t)Db * 8, stream, d); launched();
  }
}
static void sorted_finish(hipStream_t stream, LaunchCount& launched, SortedDev& d) {
  const int64_t m = (int64_t)d.L * d.S;
  hipLaunchKernelGGL(k_sorted_finish, dim3((unsigned)std::min<int64_t>(GRID_MAX, (m + SO_BLOCK - 1) / SO_BLOCK)), dim3(SO_BLOCK), 0, stream, d); launched();
}

// the plan alone (every output NULL), else uploads, per block of draws the value kernel on the block's view, the selection and the counts, then the
// finish, the summary kernels and the downloads — on `stream`, everything allocated here freed here (summary_run's discipline)
static void sorted_run(hipStream_t stream, int P, const SortedCall& c, int64_t& launches) {
  const ContrastCall& ar = c.arms;
  const bool two = c.nArms == 2;
  bool walks = true;
  SummaryCall r = two ? contrast_rows(ar, walks) : ar.rows;
  const ReadoutPlan plan = readout_plan(r, 0, two ? 8 : 4, false);
  const ChunkPlan cp = chunk_plan(r.nT, r.S, 0, QT_SCRATCH_DEFAULT, 1, 64);          // (the sort of the summary over the draws: Sp, R)
  const int64_t n = r.nT, S = r.S;
  const size_t Q = (size_t)ar.Q, L = (size_t)(c.Qr + c.J);
  // the draws of a block: what the scratch holds of whole groups of QT_GROUP draws, 8 at least, SO_DRAWS_MAX at most; all draws where they fit
  // (chunk_plan's rule with the draws in the place of the rows: a "row" of it is one draw's n values; beyond 2^30 rows the block is 8 draws anyway)
  const int64_t Db = std::min<int64_t>(SO_DRAWS_MAX, chunk_plan(S, std::min<int64_t>(n, (int64_t)1 << 30), ar.scratchBytes, SO_SCRATCH_DEFAULT, 1, QT_GROUP).C);
  const int64_t blocks = (S + Db - 1) / Db;
  SortedDev d{};
  {
    int64_t lo[SO_TARGETS_MAX], hi[SO_TARGETS_MAX]; double g[SO_TARGETS_MAX];
    for (int j = 0; j < c.Qr; ++j) {                                               // qt_type7_rows' h, lo, hi and g, across the rows
      const double h = c.rowProbs[j] * (double)(n - 1);
      lo[j] = std::min<int64_t>((int64_t)std::floor(h), n - 1); hi[j] = std::min<int64_t>(lo[j] + 1, n - 1);
      g[j] = h - (double)lo[j];
      if (g[j] == 0.0) hi[j] = lo[j];                                              // (y(hi) is not read)
    }
    for (int j = 0; j < c.J; ++j) { lo[c.Qr + j] = hi[c.Qr + j] = c.cutRank[j]; g[c.Qr + j] = 0.0; }
    sorted_targets(d, (int)L, lo, hi, g, c.J, c.cutRank);
  }
  r.info[0] = !walks ? 0 : plan.staged ? 1 : 2; r.info[1] = Db; r.info[2] = blocks; r.info[3] = 0; r.info[4] = 0; r.info[5] = S;
  r.info[6] = d.U; r.info[7] = SO_PASSES;
  if (!c.mean && !c.m2 && !c.quantiles && !c.draws && !c.nAbove && !c.nBelow) return;          // the query: the plan, nothing launched
  CallBuffers buf(stream);
  ContrastDev a{};
  if (two) contrast_upload(buf, a, ar, r, P, plan); else buf.upload_rows(a, r, P, plan.stageNodes);
  a.vals = buf.alloc<double>(nullptr, (size_t)n * (size_t)Db);
  sorted_state(buf, d, Db, S, n);
  if (c.nAbove && c.J) d.nAbove = buf.alloc<int32_t>(nullptr, (size_t)c.J * (size_t)n);
  if (c.nBelow && c.J) d.nBelow = buf.alloc<int32_t>(nullptr, (size_t)c.J * (size_t)n);
  d.out = buf.alloc<double>(nullptr, L * (size_t)S);
  LevelsSummary sum;          // D's Qr + J rows as levels of unit weight
  sum.prepare(buf, cp, S, ar.probs, c.quantiles ? ar.Q : 0, (int64_t)L);
  double* mean = c.mean ? buf.alloc<double>(nullptr, L) : nullptr;
  double* m2 = c.m2 ? buf.alloc<double>(nullptr, L) : nullptr;
  double* quantiles = c.quantiles ? buf.alloc<double>(nullptr, Q * L) : nullptr;
  arm_values_prepare(plan, two);
  LaunchCount launched{launches};
  for (int64_t kb = 0; kb < S; kb += Db) {
    const int64_t Dk = std::min<int64_t>(Db, S - kb);
    ContrastDev v = a;                                                             // the view of the block: every per-draw array advanced by kb
    v.treeStart += kb * a.T; v.scale += 2 * kb;
    if (v.denseCoef) v.denseCoef += kb * a.M;
    if (v.ellCoef) v.ellCoef += kb * a.q;
    if (two) { v.order += kb * a.T; v.numBase += kb; }
    v.S = Dk; v.numNodes = kb + Dk < S ? r.treeStart[(kb + Dk) * r.T] : (int64_t)r.numNodes;
    v.chunk0 = 0; v.chunkRows = n;
    arm_values_launch(stream, plan, chunk_grid(v), v, two); launched();
    sorted_block(stream, launched, d, a.vals, Dk, kb, (int)Dk);
  }
  sorted_finish(stream, launched, d);
  sum.run(stream, launched, d.out, (int64_t)L, 0, mean, m2, quantiles, (int64_t)L);
  if (mean) HIP_OK(hipMemcpyAsync(c.mean, mean, L * 8, hipMemcpyDeviceToHost, stream));
  if (m2) HIP_OK(hipMemcpyAsync(c.m2, m2, L * 8, hipMemcpyDeviceToHost, stream));
  if (quantiles) HIP_OK(hipMemcpyAsync(c.quantiles, quantiles, Q * L * 8, hipMemcpyDeviceToHost, stream));
  if (c.draws) HIP_OK(hipMemcpyAsync(c.draws, d.out, L * (size_t)S * 8, hipMemcpyDeviceToHost, stream));
  if (d.nAbove) HIP_OK(hipMemcpyAsync(c.nAbove, d.nAbove, (size_t)c.J * (size_t)n * 4, hipMemcpyDeviceToHost, stream));
  if (d.nBelow) HIP_OK(hipMemcpyAsync(c.nBelow, d.nBelow, (size_t)c.J * (size_t)n * 4, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  r.info[3] = launched.mine; r.info[4] = buf.bytes;
}

// TEST ENTRY (s4b_test_sorted_select): the selection and the count kernels ALONE on a caller's matrix values [n x S] row-major, in blocks of blockDraws
// columns read in place (row stride S)
static void sorted_select_test(hipStream_t stream, const SortedSelectCall& c, int64_t& launches) {
  CallBuffers buf(stream);
  const int64_t n = c.n, S = c.S, Db = std::min<int64_t>(c.blockDraws, S);
  SortedDev d{};
  {
    int64_t lo[SO_TARGETS_MAX]; double g[SO_TARGETS_MAX];
    for (int j = 0; j < c.nRanks; ++j) { lo[j] = c.ranks[j]; g[j] = 0.0; }
    sorted_targets(d, c.nRanks, lo, lo, g, c.nCuts, c.cutRank);
  }
  const double* vals = buf.alloc(c.values, (size_t)n * (size_t)S);
  sorted_state(buf, d, Db, S, n);
  if (c.nAbove && c.nCuts) d.nAbove = buf.alloc<int32_t>(nullptr, (size_t)c.nCuts * (size_t)n);
  if (c.nBelow && c.nCuts) d.nBelow = buf.alloc<int32_t>(nullptr, (size_t)c.nCuts * (size_t)n);
  d.out = buf.alloc<double>(nullptr, (size_t)std::max(1, c.nRanks) * (size_t)S);
  LaunchCount launched{launches};
  for (int64_t kb = 0; kb < S; kb += Db) sorted_block(stream, launched, d, vals + kb, S, kb, (int)std::min<int64_t>(Db, S - kb));
  if (c.nRanks) sorted_finish(stream, launched, d);
  if (c.nRanks && c.orderStats) HIP_OK(hipMemcpyAsync(c.orderStats, d.out, (size_t)c.nRanks * (size_t)S * 8, hipMemcpyDeviceToHost, stream));
  if (d.nAbove) HIP_OK(hipMemcpyAsync(c.nAbove, d.nAbove, (size_t)c.nCuts * (size_t)n * 4, hipMemcpyDeviceToHost, stream));
  if (d.nBelow) HIP_OK(hipMemcpyAsync(c.nBelow, d.nBelow, (size_t)c.nCuts * (size_t)n * 4, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  if (c.info) {
    c.info[0] = sorted_group(d.U); c.info[1] = Db; c.info[2] = (S + Db - 1) / Db; c.info[3] = launched.mine; c.info[4] = buf.bytes; c.info[5] = S;
    c.info[6] = d.U; c.info[7] = SO_PASSES;
  }
}
