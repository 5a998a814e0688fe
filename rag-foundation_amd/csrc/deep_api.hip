// deep_api.hip — C ABI of the deep search (include/rfx.h, "deep search"): the exact top-k of a flat store for k
// in 65..1,024.  Kernels: k_deep.hip (bf16 / f16) and k_deep_f32.hip (f32); plan: deep_plan.h; design: DESIGN
// §4.18 and §4.23.
#include <hip/hip_runtime.h>

#include "index_access.h"
#include "k_deep.h"
#include "k_deep_f32.h"
#include "rfx_kernels.h"

namespace {

using rfx::api_fail;

// the stores the search serves (after deep_validate passed): flat, any dtype
int deep_search_supported(int dim, int dtype, bool view) {
  if (view) return api_fail(RFX_EUNSUPPORTED, "deep search does not serve union views (search the member stores)");
  if (dtype != RFX_BF16 && dtype != RFX_F16 && dtype != RFX_F32)
    return api_fail(RFX_EUNSUPPORTED, "no deep scan kernel for dim=%d dtype=%d", dim, dtype);
  if (dim % 64 != 0 || dim > rfx::kDeepMaxDim)
    return api_fail(RFX_EUNSUPPORTED, "no deep scan kernel for dim=%d dtype=%d (dim %% 64 == 0 up to %d)", dim, dtype,
                    rfx::kDeepMaxDim);
  return RFX_OK;
}

// the stores rfx_deep_plan describes: those of the bf16 / f16 scan (an f32 store is split by the same numbers)
int deep_supported(int dim, int dtype, bool view) {
  if (!view && dtype != RFX_BF16 && dtype != RFX_F16)
    return api_fail(RFX_EUNSUPPORTED, "no deep scan kernel for dim=%d dtype=%d (bf16 and f16 stores only)", dim, dtype);
  return deep_search_supported(dim, dtype, view);
}

}  // namespace

extern "C" {

int rfx_deep_plan(int64_t rows, int dim, int dtype, int64_t nq, int k, int* out) {
  if (!out) return api_fail(RFX_EINVAL, "null output");
  const std::string err = rfx::deep_validate(rows, dim, nq, k);
  if (!err.empty()) return api_fail(RFX_EINVAL, "deep search: %s", err.c_str());
  if (const int rc = deep_supported(dim, dtype, false)) return rc;
  const rfx::DeepPlan p = rfx::deep_plan(rows, nq, k);
  out[0] = p.ranges, out[1] = p.rows_per_range, out[2] = p.kb, out[3] = p.q_per_wg;
  return RFX_OK;
}

int rfx_search_deep_workspace_bytes(rfx_index_t h, int64_t nq, int k, size_t* out_bytes) {
  if (!out_bytes) return api_fail(RFX_EINVAL, "null output");
  rfx::IndexRead ix;
  if (const int rc = rfx::api_index_read(h, &ix)) return rc;
  const std::string err = rfx::deep_validate(ix.rows, ix.dim, nq, k);
  if (!err.empty()) return api_fail(RFX_EINVAL, "deep search: %s", err.c_str());
  if (const int rc = deep_search_supported(ix.dim, ix.dtype, ix.view)) return rc;
  *out_bytes = rfx::deep_ws_bytes(rfx::deep_plan(ix.rows, nq, k), nq);
  return RFX_OK;
}

int rfx_search_deep(rfx_index_t h, const void* queries_d, int64_t nq, int k, const uint32_t* row_mask_d, float* out_scores_d,
                    int64_t* out_rows_d, void* ws_d, size_t ws_bytes, void* stream) {
  rfx::IndexRead ix;
  if (const int rc = rfx::api_index_read(h, &ix)) return rc;
  const std::string err = rfx::deep_validate(ix.rows, ix.dim, nq, k);
  if (!err.empty()) return api_fail(RFX_EINVAL, "deep search: %s", err.c_str());
  if (const int rc = deep_search_supported(ix.dim, ix.dtype, ix.view)) return rc;
  if (nq == 0) return RFX_OK;
  if (!queries_d || !out_scores_d || !out_rows_d) return api_fail(RFX_EINVAL, "null queries / outputs");
  if ((uintptr_t)queries_d & 15) return api_fail(RFX_EINVAL, "deep search: queries must be 16-byte aligned");
  const rfx::DeepPlan p = rfx::deep_plan(ix.rows, nq, k);
  const size_t need = rfx::deep_ws_bytes(p, nq);
  if (!ws_d || ws_bytes < need || ((uintptr_t)ws_d & 7))
    return api_fail(RFX_EINVAL, "workspace too small (%zu < %zu)", ws_d ? ws_bytes : (size_t)0, need);
  const hipError_t e = hipSetDevice(ix.device);
  if (e != hipSuccess) return api_fail(RFX_EDEVICE, "hipSetDevice: %s", hipGetErrorString(e));
  const int rc = ix.dtype == RFX_F32
                     ? rfx::launch_deep_search_f32(p, ix.data, ix.rows, ix.dim, queries_d, nq, k, row_mask_d, (uint64_t*)ws_d,
                                                   out_scores_d, out_rows_d, (hipStream_t)stream)
                     : rfx::launch_deep_search(p, ix.data, ix.rows, ix.dim, ix.dtype, queries_d, nq, k, row_mask_d,
                                               (uint64_t*)ws_d, out_scores_d, out_rows_d, (hipStream_t)stream);
  if (rc != 0)
    return api_fail(RFX_EUNSUPPORTED, "deep search launch rejected (dim=%d dtype=%d k=%d)", ix.dim, ix.dtype, k);
  const hipError_t e2 = hipGetLastError();
  if (e2 != hipSuccess) return api_fail(RFX_EDEVICE, "deep search: %s", hipGetErrorString(e2));
  return RFX_OK;
}

}  // extern "C"
