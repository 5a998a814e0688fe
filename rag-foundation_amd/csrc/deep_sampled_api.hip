// deep_sampled_api.hip — C ABI of the sampled-threshold deep search (include/rfx.h, "deep search, sampled
// threshold").  Kernels: k_deep_sampled.hip; plan: deep_sampled_plan.h; design: DESIGN §4.20.  Argument checks and
// error codes are rfx_search_deep's (deep_api.hip).
#include <hip/hip_runtime.h>

#include "index_access.h"
#include "k_deep_sampled.h"
#include "rfx_kernels.h"

namespace {

using rfx::api_fail;

// deep_api.hip's deep_supported, restated: the stores the kernels serve (after deep_validate passed)
int sampled_supported(int dim, int dtype, bool view) {
  if (view) return api_fail(RFX_EUNSUPPORTED, "deep search does not serve union views (search the member stores)");
  if (dtype != RFX_BF16 && dtype != RFX_F16)
    return api_fail(RFX_EUNSUPPORTED, "no deep scan kernel for dim=%d dtype=%d (bf16 and f16 stores only)", dim, dtype);
  if (dim % 64 != 0 || dim > rfx::kDeepMaxDim)
    return api_fail(RFX_EUNSUPPORTED, "no deep scan kernel for dim=%d dtype=%d (dim %% 64 == 0 up to %d)", dim, dtype,
                    rfx::kDeepMaxDim);
  return RFX_OK;
}

int sampled_check(int64_t rows, int dim, int dtype, bool view, int64_t nq, int k) {
  const std::string err = rfx::deep_validate(rows, dim, nq, k);
  if (!err.empty()) return api_fail(RFX_EINVAL, "deep search: %s", err.c_str());
  return sampled_supported(dim, dtype, view);
}

}  // namespace

extern "C" {

int rfx_deep_sampled_plan(int64_t rows, int dim, int dtype, int64_t nq, int k, int* out) {
  if (!out) return api_fail(RFX_EINVAL, "null output");
  if (const int rc = sampled_check(rows, dim, dtype, false, nq, k)) return rc;
  const rfx::DeepSampledPlan p = rfx::deep_sampled_plan(rows, dim, nq, k);
  out[0] = p.dense, out[1] = p.S, out[2] = p.stride, out[3] = p.cap, out[4] = p.q_per_wg, out[5] = p.ranges;
  return RFX_OK;
}

int rfx_search_deep_sampled_workspace_bytes(rfx_index_t h, int64_t nq, int k, size_t* out_bytes) {
  if (!out_bytes) return api_fail(RFX_EINVAL, "null output");
  rfx::IndexRead ix;
  if (const int rc = rfx::api_index_read(h, &ix)) return rc;
  if (const int rc = sampled_check(ix.rows, ix.dim, ix.dtype, ix.view, nq, k)) return rc;
  *out_bytes = rfx::deep_sampled_ws_bytes(rfx::deep_sampled_plan(ix.rows, ix.dim, nq, k), ix.rows, ix.dim, nq, k);
  return RFX_OK;
}

int rfx_search_deep_sampled(rfx_index_t h, const void* queries_d, int64_t nq, int k, const uint32_t* row_mask_d,
                            float* out_scores_d, int64_t* out_rows_d, void* ws_d, size_t ws_bytes, void* stream) {
  rfx::IndexRead ix;
  if (const int rc = rfx::api_index_read(h, &ix)) return rc;
  if (const int rc = sampled_check(ix.rows, ix.dim, ix.dtype, ix.view, nq, k)) return rc;
  if (nq == 0) return RFX_OK;
  if (!queries_d || !out_scores_d || !out_rows_d) return api_fail(RFX_EINVAL, "null queries / outputs");
  if ((uintptr_t)queries_d & 15) return api_fail(RFX_EINVAL, "deep search: queries must be 16-byte aligned");
  const rfx::DeepSampledPlan p = rfx::deep_sampled_plan(ix.rows, ix.dim, nq, k);
  const size_t need = rfx::deep_sampled_ws_bytes(p, ix.rows, ix.dim, nq, k);
  if (!ws_d || ws_bytes < need || ((uintptr_t)ws_d & 255))
    return api_fail(RFX_EINVAL, "workspace too small or not 256-byte aligned (%zu < %zu)", ws_d ? ws_bytes : (size_t)0, need);
  const hipError_t e = hipSetDevice(ix.device);
  if (e != hipSuccess) return api_fail(RFX_EDEVICE, "hipSetDevice: %s", hipGetErrorString(e));
  if (rfx::launch_deep_sampled_search(p, ix.data, ix.rows, ix.dim, ix.dtype, queries_d, nq, k, row_mask_d, (uint8_t*)ws_d,
                                      out_scores_d, out_rows_d, (hipStream_t)stream) != 0)
    return api_fail(RFX_EUNSUPPORTED, "sampled deep search launch rejected (dim=%d dtype=%d k=%d)", ix.dim, ix.dtype, k);
  const hipError_t e2 = hipGetLastError();
  if (e2 != hipSuccess) return api_fail(RFX_EDEVICE, "sampled deep search: %s", hipGetErrorString(e2));
  return RFX_OK;
}

}  // extern "C"
