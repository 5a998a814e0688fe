// k_scan_mfma8.hip — plan + dispatch of the k-split d = 1024 batched scan (kernel: k_scan_mfma8.h,
// instantiated per dtype in k8_*.hip).  Same grid, lists and threshold table as kernel 7.
#include "k_scan_mfma8.h"

namespace rfx {
namespace k8 {
#define RFX_K8_DECL(NAME)                                                                                 \
  int NAME(int kl, dim3 grid, hipStream_t st, const uint16_t* X, const uint16_t* Qp, int nq, int ntiles,     \
           int ranges, int groups, int paired, uint32_t* tau, float* cs, int* cr, int64_t n_lists,        \
           const uint32_t* mask, int mask_words, const uint32_t* gate);
RFX_K8_DECL(launch_bf16_1024)
RFX_K8_DECL(launch_f16_1024)
#undef RFX_K8_DECL
}  // namespace k8

static size_t tau_bytes_mfma8(const MfmaPlan& p) { return (size_t)p.nq_pad * k8::kTauW * sizeof(uint32_t); }

// 128 queries per workgroup, the groups of a range on one XCD.  p.blocks = R, p.q_blocks = G; one-dimensional grid.
static MfmaPlan plan_scan_mfma8(int64_t nrows, int D, int dtype, int64_t nq, int k) {
  return plan_scan_ranges((dtype == RFX_BF16 || dtype == RFX_F16) && D == 1024, k8::kQG, k8::kTM, k8::kListsPerBlock,
                          32, true, nrows, nq, k);
}

static int launch_scan_mfma8(const MfmaPlan& p, const void* X, int nrows, int D, int dtype, const void* Qpad, int nq,
                             uint32_t* tau, float* cs, int* cr, hipStream_t st, const uint32_t* mask,
                             const uint32_t* gate, bool tau_zeroed) {
  static_assert(k8::kTauW == kFallbackTauW, "screen_queries_kernel zeroes this table for the gated fallback");
  if (!p.ok || D != 1024) return -1;
  const int ntiles = (nrows + k8::kTM - 1) / k8::kTM;
  if (!tau_zeroed && hipMemsetAsync(tau, 0, tau_bytes_mfma8(p), st) != hipSuccess) return -2;
  const int paired = p.blocks % 8 == 0 ? 1 : 0;
  dim3 grid(p.blocks * p.q_blocks);
  auto f = dtype == RFX_BF16 ? k8::launch_bf16_1024 : k8::launch_f16_1024;
  return f(p.k_lane, grid, st, (const uint16_t*)X, (const uint16_t*)Qpad, nq, ntiles, p.blocks, p.q_blocks,
           paired, tau, cs, cr, p.n_lists, mask, (nrows + 31) / 32, gate);
}

const ExactScan& exact_scan_mfma8() {
  static const ExactScan s{8, 2, plan_scan_mfma8, tau_bytes_mfma8, launch_scan_mfma8};
  return s;
}

}  // namespace rfx
