// k_lex_score.h — the BM25 score of one row for the questions of a group: device code shared by
// the lexical scans (k_lex.hip: top-k up to 64; k_lex_deep.hip: 65..1,024).  ONE definition, so that every scan
// gives a row the same score bits: one f64 division per entry, contraction off, the same butterfly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rfx_device.h"

namespace rfx {

// One entry's contribution to the questions of the group: x = (tf * (k1 + 1)) / (tf + B_r), an IEEE f64
// division taken once per entry (it does not depend on the question), then acc_q += w_q * x with the product
// and the sum rounded on their own.
template <int NQT>
__device__ __forceinline__ void lex_accumulate(uint32_t e, double B, double k1p1, const float* __restrict__ wt,
                                               double (&acc)[NQT]) {
#pragma clang fp contract(off)
  const uint32_t tf = e >> 16;
  if (tf == 0u) return;  // no entry in this lane (a stored tf is >= 1)
  const float* wp = wt + (size_t)(e & 0xffffu) * NQT;
  float w[NQT];
  if constexpr (NQT == 8) {
    const float4 a = ((const float4*)wp)[0], b4 = ((const float4*)wp)[1];
    w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b4.x, w[5] = b4.y, w[6] = b4.z, w[7] = b4.w;
  } else {
#pragma unroll
    for (int q = 0; q < NQT; ++q) w[q] = wp[q];
  }
  bool any = false;
#pragma unroll
  for (int q = 0; q < NQT; ++q) any |= w[q] != 0.0f;
  if (!any) return;
  const double tfd = (double)tf;
  const double num = tfd * k1p1;
  const double den = tfd + B;
  const double x = num / den;
#pragma unroll
  for (int q = 0; q < NQT; ++q) {
    const double t = (double)w[q] * x;
    acc[q] = acc[q] + t;
  }
}

// The xor butterfly (32, 16, 8, 4, 2, 1) over NQT sums at once: at each of the first log2(NQT) steps a lane
// keeps half of its sums and hands the other half to its partner, so question q's sum pairs the same lanes in
// the same order as a butterfly over that sum alone (f64 addition commutes: the value is the lone butterfly's,
// whatever NQT).  Afterwards acc[0] of lane l is the sum of question lex_owner_q(l).
template <int NQT>
__device__ __forceinline__ double lex_reduce(double (&acc)[NQT], int lane) {
  int off = 32;
#pragma unroll
  for (int n = NQT; n > 1; n >>= 1) {
    const int half = n >> 1;
    const bool hi = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const double keep = hi ? acc[i + half] : acc[i];
      const double send = hi ? acc[i] : acc[i + half];
      acc[i] = keep + __shfl_xor(send, off);
    }
    off >>= 1;
  }
  for (; off; off >>= 1) acc[0] = acc[0] + __shfl_xor(acc[0], off);
  return acc[0];
}
// the first lane that holds question q's sum after lex_reduce
template <int NQT>
__device__ __forceinline__ int lex_owner_lane(int q) {
  int l = 0, off = 32;
  for (int n = NQT; n > 1; n >>= 1) {
    if (q & (n >> 1)) l |= off;
    off >>= 1;
  }
  return l;
}

__device__ __forceinline__ long long readlane_i64(long long v, int l) {
  return (long long)(((uint64_t)(uint32_t)readlane_i((int)(v >> 32), l) << 32) | (uint32_t)readlane_i((int)v, l));
}

}  // namespace rfx
