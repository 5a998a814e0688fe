// k_cand_keys.h — the candidate key of the deep searches (k in 65..1,024: k_deep, k_deep_sampled, k_ivf_deep,
// k_lex_deep, k_deep_select) and the LDS routines that work on buffers of such keys.  Device code, gfx950 only.
//
// A candidate is one u64 key: (ord_f32(score + 0.0f) << 32) | ~row.  A larger key is a better candidate under the
// ranking rule (score desc, row asc), so one unsigned compare carries the tie-break through every step.  s + 0
// folds -0 into +0, which compare equal as floats; a score decoded from a key is therefore never -0.0 (and for
// s > 0, the BM25 scores, s + 0 has the bits of s).  Key 0 is "none": it lies below the key of every real score,
// -inf included, so a buffer padded with zeros sorts its candidates to the front.  A NaN score (a tombstoned row) gets no key: the callers test for it.
#pragma once
#include "rfx_device.h"

namespace rfx {

__device__ __forceinline__ uint64_t cand_key(float s, int row) {
  return ((uint64_t)ord_f32(s + 0.0f) << 32) | (uint32_t)~(uint32_t)row;
}
__device__ __forceinline__ float cand_key_score(uint64_t key) { return unord_f32((uint32_t)(key >> 32)); }
__device__ __forceinline__ int cand_key_row(uint64_t key) { return (int)~(uint32_t)key; }

// Workgroup-wide: keys[0 .. k) -> question q's k outputs, (score, int64 row), or (-inf, -1) for key 0.
__device__ __forceinline__ void cand_write(const uint64_t* keys, int64_t q, int k, float* __restrict__ out_s,
                                           int64_t* __restrict__ out_r) {
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    const uint64_t key = keys[j];
    out_s[q * k + j] = key ? cand_key_score(key) : -__builtin_inff();
    out_r[q * k + j] = key ? (int64_t)cand_key_row(key) : -1;
  }
}

// Wave-wide (every lane calls it).  The passing lanes among `mine` (the lanes that hold this lane's buffer, itself
// included; ~0 when the wave fills one buffer) claim consecutive slots of it: one ballot, a prefix count, one LDS
// add by the first of them.  Returns the lane's slot, or -1.  The caller checks the slot against the buffer's size.
__device__ __forceinline__ int cand_claim(bool pass, uint64_t mine, int* cnt) {
  const int lane = lane_id();
  const uint64_t m = __ballot(pass) & mine;
  const int leader = m ? __builtin_ctzll(m) : lane;
  int base = 0;
  if (pass && lane == leader) base = atomicAdd(cnt, __popcll(m));
  base = __shfl(base, leader);
  return pass ? base + __popcll(m & ((1ull << lane) - 1)) : -1;
}

// Workgroup-wide: the buffers named in `need` (uniform; buffer i at buf + i * stride), n keys each (a power of
// two), sorted best first.  Bitonic, in place; the caller's writes are behind a barrier, and it ends on one.
__device__ __forceinline__ void cand_sort(uint64_t* buf, int stride, uint32_t need, int n) {
  for (int k2 = 2; k2 <= n; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (uint32_t m = need; m; m &= m - 1) {
        uint64_t* b = buf + (size_t)__builtin_ctz(m) * stride;
        for (int i = threadIdx.x; i < n / 2; i += blockDim.x) {
          const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
          const uint64_t a = b[lo], c = b[hi];
          if ((a < c) == ((lo & k2) == 0)) {
            b[lo] = c;
            b[hi] = a;
          }
        }
      }
      __syncthreads();
    }
}

// Workgroup-wide: the cut of the buffers named in `need` (uniform, at most 32; buffer i holds min(cnt[i], cap) keys
// at buf + i * cap, cap a power of two > kb).  Each is padded with key 0 and sorted; its kb best stay, cnt[i] <-
// min(cnt[i], kb), tau[i] <- the kb-th key (0 while fewer are held).  Every wave is here and the appends are behind
// a barrier: nothing is appended meanwhile.  Ends on a barrier.
__device__ __forceinline__ void cand_cut(uint64_t* buf, int cap, int kb, uint32_t need, int* cnt, uint64_t* tau) {
  for (uint32_t m = need; m; m &= m - 1) {
    const int i = __builtin_ctz(m);
    for (int e = min(cnt[i], cap) + (int)threadIdx.x; e < cap; e += blockDim.x) buf[(size_t)i * cap + e] = 0;
  }
  __syncthreads();
  cand_sort(buf, cap, need, cap);
  if (threadIdx.x < 32 && ((need >> threadIdx.x) & 1u)) {
    cnt[threadIdx.x] = min(cnt[threadIdx.x], kb);
    tau[threadIdx.x] = buf[(size_t)threadIdx.x * cap + kb - 1];
  }
  __syncthreads();
}

}  // namespace rfx
