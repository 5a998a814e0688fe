// k_deep_buf.h — the LDS candidate buffers of the deep scans (k_deep.hip: bf16 / f16; k_deep_f32.hip: f32) and of
// their merge: layout, the workgroup's meeting, and the launch checks both scans share.  Keys and the sort:
// k_cand_keys.h; design: DESIGN §4.18.
#pragma once
#include "deep_plan.h"
#include "k_cand_keys.h"

namespace rfx {

constexpr int kDeepQSlots = 16;  // threshold / count slots of a workgroup (questions per workgroup <= 16)

// LDS of a workgroup: nqg buffers of 2 * KB keys, then the thresholds (keys; 0 = none yet) and the fills.
struct DeepBuf {
  uint64_t* buf;
  uint64_t* tau;
  int* cnt;
  int KB;
  __device__ __forceinline__ DeepBuf(uint64_t* lds, int nqg, int kb)
      : buf(lds), tau(lds + (size_t)nqg * 2 * kb), cnt((int*)(lds + (size_t)nqg * 2 * kb + kDeepQSlots)), KB(kb) {}
};
inline size_t deep_lds_bytes(int nqg, int kb) { return (size_t)nqg * 2 * kb * 8 + kDeepQSlots * 8 + kDeepQSlots * 4; }

// Workgroup-wide meeting after a round of appends.  Every buffer that holds more than `lim` keys is sorted, its
// KB best stay and the KB-th becomes its threshold (lim = -1: every buffer, the final cut).  Returns the buffers
// it cut (uniform).  Nothing may be appended between the entry and the return.
__device__ __forceinline__ uint32_t deep_compact(const DeepBuf& B, int nqg, int lim) {
  const int N = 2 * B.KB;
  __syncthreads();  // the round's appends are in
  uint32_t need = 0;
  for (int q = 0; q < nqg; ++q) need |= (B.cnt[q] > lim ? 1u : 0u) << q;
  __syncthreads();  // every thread has read the fills before anyone appends again
  if (!need) return 0;
  cand_cut(B.buf, N, B.KB, need, B.cnt, B.tau);
  return need;
}

// The arguments a scan launch accepts, whatever the store's type (host).
inline bool deep_launch_ok(const DeepPlan& p, int64_t nrows, int D, int64_t nq, int k) {
  if (D < 64 || D > kDeepMaxDim || D % 64 != 0) return false;
  if (nq < 1 || nq > kDeepMaxNq || k < kDeepMinK || k > p.kb || nrows < 0 || nrows > 0x7fffffffll - 1) return false;
  return p.ranges >= 1 && p.check_rounds >= 2 && p.check_rounds % 2 == 0 && 2 * p.kb >= p.kb + p.check_rounds * kDeepRound &&
         p.q_per_wg <= kDeepQSlots && (int64_t)(p.ranges - 1) * p.rows_per_range <= nrows &&
         deep_lds_bytes(p.q_per_wg, p.kb) <= (size_t)kDeepLdsBudget;
}

}  // namespace rfx
