// k_scan_mfma9.hip — plan + dispatch of the batched f32 scan (kernel: k_scan_mfma9.h, instantiated
// in k9_f32_768.hip).
#include "k_scan_mfma9.h"

namespace rfx {
namespace k9 {
int launch_f32_768(int kl, dim3 grid, hipStream_t st, const float* X, const float* Qp, int nq, int ntiles,
                   int ranges, int groups, int paired, uint32_t* tau, float* cs, int* cr, int64_t n_lists,
                   const uint32_t* mask, int mask_words, const uint32_t* gate);
}  // namespace k9

static size_t tau_bytes_mfma9(const MfmaPlan& p) { return (size_t)p.nq_pad * k9::kTauW * sizeof(uint32_t); }

// f32 stores, 16 < nq: 128 queries per workgroup, the groups of a range on one XCD.  Below 17 queries the VALU
// scan's 8-query slices cost less than a 128-query MFMA pass (the kernel computes all 128 columns).
static MfmaPlan plan_scan_mfma9(int64_t nrows, int D, int dtype, int64_t nq, int k) {
  return plan_scan_ranges(dtype == RFX_F32 && D == 768 && nq > 16, k9::kQG, k9::kTM, k9::kListsPerBlock, 32, true,
                          nrows, nq, k);
}

static int launch_scan_mfma9(const MfmaPlan& p, const void* X, int nrows, int D, int dtype, const void* Qpad, int nq,
                             uint32_t* tau, float* cs, int* cr, hipStream_t st, const uint32_t* mask,
                             const uint32_t* gate, bool tau_zeroed) {
  static_assert(k9::kTauW == kFallbackTauW, "screen_queries_kernel zeroes this table for the gated fallback");
  if (!p.ok || D != 768 || dtype != RFX_F32) return -1;
  const int ntiles = (nrows + k9::kTM - 1) / k9::kTM;
  if (!tau_zeroed && hipMemsetAsync(tau, 0, tau_bytes_mfma9(p), st) != hipSuccess) return -2;
  const int paired = p.blocks % 8 == 0 ? 1 : 0;
  dim3 grid(p.blocks * p.q_blocks);
  return k9::launch_f32_768(p.k_lane, grid, st, (const float*)X, (const float*)Qpad, nq, ntiles, p.blocks,
                            p.q_blocks, paired, tau, cs, cr, p.n_lists, mask, (nrows + 31) / 32, gate);
}

// f32 stores: batched scan on v_mfma_f32_16x16x4_f32
const ExactScan& exact_scan_mfma9() {
  static const ExactScan s{9, 4, plan_scan_mfma9, tau_bytes_mfma9, launch_scan_mfma9};
  return s;
}

}  // namespace rfx
