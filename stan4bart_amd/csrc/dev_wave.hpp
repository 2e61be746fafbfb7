// Shared by both translation units of libs4b.so (dev_hip.hip, dev_sweep.hip): the wave reductions.  Templates and forceinline
// functions only: nothing here is defined twice at link time.
#ifndef S4B_DEV_WAVE_HPP
#define S4B_DEV_WAVE_HPP

#include <hip/hip_runtime.h>

namespace s4b {

// ------------------------------------------------------------------------------------------------
// wave / block reductions with a fixed order (deterministic)
// value of lane (l ^ O), O a power of two: register-to-register on gfx950 (DPP within rows of 16 lanes, the permlane swaps across
// them) instead of a trip through the LDS crossbar (ds_bpermute) — the dependent exchange chains of the reductions are several
// times shorter
template <int O>
__device__ __forceinline__ int wave_xor(int v) {
  static_assert(O == 1 || O == 2 || O == 4 || O == 8 || O == 16 || O == 32, "power of two below 64");
  if constexpr (O == 1) return __builtin_amdgcn_update_dpp(0, v, 0xb1, 0xf, 0xf, false);           // quad_perm [1,0,3,2]
  else if constexpr (O == 2) return __builtin_amdgcn_update_dpp(0, v, 0x4e, 0xf, 0xf, false);      // quad_perm [2,3,0,1]
  else if constexpr (O == 4) {   // lanes with bit 2 clear read lane + 4 (row_shl:4), the others lane - 4 (row_shr:4)
    const int a = __builtin_amdgcn_update_dpp(0, v, 0x104, 0xf, 0x5, false);
    return __builtin_amdgcn_update_dpp(a, v, 0x114, 0xf, 0xa, false);
  } else if constexpr (O == 8) return __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false);   // row_ror:8
  else if constexpr (O == 16) {
    const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);   // {odd rows <- even rows of the copy, even rows <- odd rows}
    return ((threadIdx.x & 16) != 0) ? (int)r[0] : (int)r[1];
  } else {
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return ((threadIdx.x & 32) != 0) ? (int)r[0] : (int)r[1];
  }
}
template <int O>
__device__ __forceinline__ double wave_xor(double v) {
  return __hiloint2double(wave_xor<O>(__double2hiint(v)), wave_xor<O>(__double2loint(v)));
}
__device__ __forceinline__ double wave_sum(double v) {   // same pairing and order as the xor butterfly 32, 16, ..., 1
  v += wave_xor<32>(v); v += wave_xor<16>(v); v += wave_xor<8>(v); v += wave_xor<4>(v); v += wave_xor<2>(v); v += wave_xor<1>(v);
  return v;
}
// NB independent sums over the 64 lanes at once: each halving step keeps one half of the values and hands the
// other half to the partner lane, so the cross-lane traffic is NB-1 + log2(64/NB) exchanges instead of 6 NB.
// Afterwards v[0] of lane l is the wave total of value wave_bin_of_lane<NB>(l).  Fixed order: deterministic.
template <int CNT, int O, int NB, class T>
__device__ __forceinline__ void wave_sum_bins_step(T (&v)[NB], int lane) {
  if constexpr (CNT > 1) {
    constexpr int h = CNT / 2;
    const bool upper = (lane & O) != 0;
#pragma unroll
    for (int j = 0; j < h; ++j) {
      const T send = upper ? v[j] : v[j + h];
      const T keep = upper ? v[j + h] : v[j];
      v[j] = keep + wave_xor<O>(send);
    }
    wave_sum_bins_step<h, O / 2, NB, T>(v, lane);
  } else if constexpr (O > 0) {
    v[0] += wave_xor<O>(v[0]);
    wave_sum_bins_step<1, O / 2, NB, T>(v, lane);
  }
}
template <int NB, class T>
__device__ __forceinline__ void wave_sum_bins(T (&v)[NB], int lane) { wave_sum_bins_step<NB, 32, NB, T>(v, lane); }
template <int NB>
__device__ __forceinline__ int wave_bin_of_lane(int lane) {
  // NB = 2^q: the q halving steps use lane bits 5, 4, ..., 6-q for value-index bits q-1, ..., 0
  constexpr int q = NB == 16 ? 4 : NB == 8 ? 3 : NB == 4 ? 2 : NB == 2 ? 1 : 0;
  return q == 0 ? 0 : (lane >> (6 - q)) & (NB - 1);
}
__device__ __forceinline__ double wave_min(double v) {
  v = fmin(v, wave_xor<32>(v)); v = fmin(v, wave_xor<16>(v)); v = fmin(v, wave_xor<8>(v)); v = fmin(v, wave_xor<4>(v)); v = fmin(v, wave_xor<2>(v)); v = fmin(v, wave_xor<1>(v));
  return v;
}
// the lexicographic minimum of the pairs (v, idx) over the 64 lanes, in every lane: the smallest v, among equal v the lowest idx (no NaN among the v)
template <int O>
__device__ __forceinline__ void wave_argmin_step(double& v, int& idx) {
  const double ov = wave_xor<O>(v);
  const int oi = wave_xor<O>(idx);
  if (ov < v || (ov == v && oi < idx)) { v = ov; idx = oi; }
}
__device__ __forceinline__ void wave_argmin(double& v, int& idx) {
  wave_argmin_step<32>(v, idx); wave_argmin_step<16>(v, idx); wave_argmin_step<8>(v, idx); wave_argmin_step<4>(v, idx); wave_argmin_step<2>(v, idx); wave_argmin_step<1>(v, idx);
}
__device__ __forceinline__ double wave_max(double v) {
  v = fmax(v, wave_xor<32>(v)); v = fmax(v, wave_xor<16>(v)); v = fmax(v, wave_xor<8>(v)); v = fmax(v, wave_xor<4>(v)); v = fmax(v, wave_xor<2>(v)); v = fmax(v, wave_xor<1>(v));
  return v;
}

}  // namespace s4b
#endif
