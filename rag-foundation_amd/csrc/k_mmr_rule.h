// k_mmr_rule.h — the device pieces of the MMR rule that every selection kernel shares: the NaN
// test of a row piece, the exact widening of a piece, and the objective.  Kernels: k_mmr.hip (up to 64
// candidates), k_mmr_deep.hip (65..1,024).
#pragma once
#include "../../include/rfx.h"
#include "rfx_device.h"

namespace rfx {
namespace mmr {

// does a 16-byte piece of a row hold a NaN?
template <int DT>
__device__ __forceinline__ bool piece_has_nan(const uint4& u) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
  bool bad = false;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (DT == RFX_F32) {
      bad |= (w[i] & 0x7fffffffu) > 0x7f800000u;
    } else {
      constexpr uint32_t inf = DT == RFX_BF16 ? 0x7f80u : 0x7c00u;
      bad |= (w[i] & 0x7fffu) > inf || ((w[i] >> 16) & 0x7fffu) > inf;
    }
  }
  return bad;
}

template <int DT>
__device__ __forceinline__ float half_to_f32(uint32_t h) {
  return DT == RFX_BF16 ? bf16_to_f32((uint16_t)h) : f16_to_f32((uint16_t)h);
}

// the 8 elements of a 16-byte piece of a 16-bit row, widened to f32
template <int DT>
__device__ __forceinline__ void widen8(const uint4& a, float (&e)[8]) {
  const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    e[2 * i] = half_to_f32<DT>(w[i] & 0xffffu);
    e[2 * i + 1] = half_to_f32<DT>(w[i] >> 16);
  }
}

// elements [8 * c8, 8 * c8 + 8) of the row at `row` (LDS or global), widened to f32
template <int DT, class P>
__device__ __forceinline__ void load8(P row, int c8, float (&e)[8]) {
  if constexpr (DT == RFX_F32) {
    const uint4 a = ((const uint4*)row)[2 * c8], b = ((const uint4*)row)[2 * c8 + 1];
    e[0] = __uint_as_float(a.x), e[1] = __uint_as_float(a.y), e[2] = __uint_as_float(a.z), e[3] = __uint_as_float(a.w);
    e[4] = __uint_as_float(b.x), e[5] = __uint_as_float(b.y), e[6] = __uint_as_float(b.z), e[7] = __uint_as_float(b.w);
  } else {
    widen8<DT>(((const uint4*)row)[c8], e);
  }
}

// obj = L * s - (1 - L) * m in f64, each operation rounded on its own
__device__ __forceinline__ double mmr_objective(double L, float s, float m) {
#pragma clang fp contract(off)
  const double rel = L * (double)s;
  const double pen = (1.0 - L) * (double)m;
  return rel - pen;
}

}  // namespace mmr
}  // namespace rfx
