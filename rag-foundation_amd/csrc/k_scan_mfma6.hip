// k_scan_mfma6.hip — plan + dispatch of the headline scan (kernel: k_scan_mfma6.h, instantiated per
// dtype in k6_*.hip).
#include "k_scan_mfma6.h"

namespace rfx {
namespace k6 {
#define RFX_K6_DECL(NAME)                                                                                 \
  int NAME(int kl, dim3 grid, hipStream_t st, const uint16_t* X, const uint16_t* Qp, int nq, int ntiles,     \
           uint32_t* tau, float* cs, int* cr, int64_t n_lists, const uint32_t* mask, const uint32_t* gate);
RFX_K6_DECL(launch_bf16_768)
RFX_K6_DECL(launch_f16_768)
#undef RFX_K6_DECL
}  // namespace k6

// threshold table: [nq_pad][kTauW] u32 (k_scan_mfma6.h; the debug build's kernel-5 ablations use the same table)
static size_t tau_bytes_mfma6(const MfmaPlan& p) { return (size_t)p.nq_pad * k6::kTauW * sizeof(uint32_t); }

// 256 queries per workgroup, one workgroup per CU: grid (ranges, q_blocks)
static MfmaPlan plan_scan_mfma6(int64_t nrows, int D, int dtype, int64_t nq, int k) {
  return plan_scan_ranges((dtype == RFX_BF16 || dtype == RFX_F16) && D == 768, k6::kQG, k6::kTM, 2, 256, false, nrows,
                          nq, k);
}

static int launch_scan_mfma6(const MfmaPlan& p, const void* X, int nrows, int D, int dtype, const void* Qpad, int nq,
                             uint32_t* tau, float* cs, int* cr, hipStream_t st, const uint32_t* mask,
                             const uint32_t* gate, bool tau_zeroed) {
  static_assert(k6::kTauW == kFallbackTauW, "screen_queries_kernel zeroes this table for the gated fallback");
  if (!p.ok || D != 768) return -1;
  const int ntiles = (nrows + k6::kTM - 1) / k6::kTM;
  if (!tau_zeroed && hipMemsetAsync(tau, 0, tau_bytes_mfma6(p), st) != hipSuccess) return -2;
  dim3 grid(p.blocks, p.q_blocks);
  auto f = dtype == RFX_BF16 ? k6::launch_bf16_768 : k6::launch_f16_768;
  return f(p.k_lane, grid, st, (const uint16_t*)X, (const uint16_t*)Qpad, nq, ntiles, tau, cs, cr, p.n_lists, mask, gate);
}

const ExactScan& exact_scan_mfma6() {
  static const ExactScan s{6, 2, plan_scan_mfma6, tau_bytes_mfma6, launch_scan_mfma6};
  return s;
}

}  // namespace rfx
