// mmr_deep_api.hip — C ABI of the deep MMR selection (include/rfx.h, "diversified retrieval at depth"): the
// rule of rfx_mmr_select over 65..1,024 candidates.  Kernels: k_mmr_deep.hip; plan: mmr_deep_plan.h; design:
// DESIGN §4.22.
#include <hip/hip_runtime.h>

#include "index_access.h"
#include "k_mmr_deep.h"
#include "rfx_kernels.h"

namespace {

using rfx::api_fail;

// the stores the kernels serve (after mmr_deep_validate passed); a union view is served as rfx_mmr_select
// serves it: the NaN gaps between its members are padding
int mmr_deep_supported(int dim, int dtype) {
  if (dtype != RFX_BF16 && dtype != RFX_F16)
    return api_fail(RFX_EUNSUPPORTED, "no deep mmr kernel for dim=%d dtype=%d (bf16 and f16 stores only)", dim, dtype);
  if (dim % 64 != 0 || dim > rfx::kMmrDeepMaxDim)
    return api_fail(RFX_EUNSUPPORTED, "no deep mmr kernel for dim=%d dtype=%d (dim %% 64 == 0 up to %d)", dim, dtype,
                    rfx::kMmrDeepMaxDim);
  return RFX_OK;
}

struct Tables {
  const float* lam;
  const int32_t* nc;
  int64_t nq;
  int n_cand_max;
};
void fill_tables(uint8_t* stage, void* ctx) {
  const Tables& t = *(const Tables*)ctx;
  float* lam_s = (float*)stage;
  int32_t* nc_s = (int32_t*)(stage + (size_t)t.nq * sizeof(float));
  for (int64_t q = 0; q < t.nq; ++q) {
    lam_s[q] = t.lam ? t.lam[q] : 0.5f;
    nc_s[q] = t.nc ? t.nc[q] : t.n_cand_max;
  }
}

}  // namespace

extern "C" {

int rfx_mmr_deep_plan(int64_t nq, int n_cand_max, int64_t* out) {
  if (!out) return api_fail(RFX_EINVAL, "null output");
  const std::string err = rfx::mmr_deep_validate(nq, n_cand_max, 1);
  if (!err.empty()) return api_fail(RFX_EINVAL, "deep mmr select: %s", err.c_str());
  const rfx::MmrDeepPlan p = rfx::mmr_deep_plan(nq, n_cand_max);
  out[0] = p.n_pad, out[1] = p.pairs, out[2] = p.slice_q, out[3] = p.slices, out[4] = (int64_t)p.total;
  return RFX_OK;
}

int rfx_mmr_deep_workspace_bytes(rfx_index_t h, int64_t nq, int n_cand_max, size_t* out_bytes) {
  if (!out_bytes) return api_fail(RFX_EINVAL, "null output");
  rfx::IndexRead ix;
  if (const int rc = rfx::api_index_read(h, &ix)) return rc;
  const std::string err = rfx::mmr_deep_validate(nq, n_cand_max, 1);
  if (!err.empty()) return api_fail(RFX_EINVAL, "deep mmr select: %s", err.c_str());
  if (const int rc = mmr_deep_supported(ix.dim, ix.dtype)) return rc;
  *out_bytes = rfx::mmr_deep_plan(nq, n_cand_max).total;
  return RFX_OK;
}

int rfx_mmr_select_deep(rfx_index_t h, const void* queries_d, int64_t nq, int n_cand_max, int k, const float* lambda_h,
                        const int32_t* n_cand_h, const float* cand_scores_d, const int64_t* cand_rows_d,
                        float* out_scores_d, int64_t* out_rows_d, float* out_obj_d, void* ws_d, size_t ws_bytes,
                        void* stream) {
  (void)queries_d;  // the candidates carry their scores: the queries are not read again
  rfx::IndexRead ix;
  if (const int rc = rfx::api_index_read(h, &ix)) return rc;
  const std::string err = rfx::mmr_deep_validate(nq, n_cand_max, k);
  if (!err.empty()) return api_fail(RFX_EINVAL, "deep mmr select: %s", err.c_str());
  if (lambda_h)
    for (int64_t q = 0; q < nq; ++q)
      if (!(lambda_h[q] >= 0.0f && lambda_h[q] <= 1.0f))  // (a NaN fails both compares)
        return api_fail(RFX_EINVAL, "lambda[%lld]=%g outside [0, 1]", (long long)q, (double)lambda_h[q]);
  if (n_cand_h)
    for (int64_t q = 0; q < nq; ++q)
      if (n_cand_h[q] < 1 || n_cand_h[q] > n_cand_max)
        return api_fail(RFX_EINVAL, "n_cand[%lld]=%d outside [1, %d]", (long long)q, (int)n_cand_h[q], n_cand_max);
  if (!cand_scores_d || !cand_rows_d || !out_scores_d || !out_rows_d) return api_fail(RFX_EINVAL, "null candidates / outputs");
  if (const int rc = mmr_deep_supported(ix.dim, ix.dtype)) return rc;
  const rfx::MmrDeepPlan p = rfx::mmr_deep_plan(nq, n_cand_max);
  if (!ws_d || ws_bytes < p.total) return api_fail(RFX_EINVAL, "workspace too small (%zu < %zu)", ws_d ? ws_bytes : (size_t)0, p.total);
  if ((uintptr_t)ws_d & 255) return api_fail(RFX_EINVAL, "deep mmr select: workspace must be 256-byte aligned");
  const hipError_t e = hipSetDevice(ix.device);
  if (e != hipSuccess) return api_fail(RFX_EDEVICE, "hipSetDevice: %s", hipGetErrorString(e));
  hipStream_t st = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)ws_d;
  Tables tb{lambda_h, n_cand_h, nq, n_cand_max};
  if (const int rc = rfx::api_stage_tables(ix, p.tables, fill_tables, &tb, ws + p.lam, st)) return rc;
  // Gram + select per slice, one after the other on the caller's stream: the slices share the scratch
  for (int64_t q0 = 0; q0 < nq; q0 += p.slice_q) {
    const int qs = (int)std::min<int64_t>(p.slice_q, nq - q0);
    if (rfx::launch_mmr_deep(p, ix.data, ix.data ? ix.rows : 0, ix.dim, ix.dtype, qs, n_cand_max, k,
                             (const float*)(ws + p.lam) + q0, (const int*)(ws + p.ncand) + q0,
                             cand_scores_d + q0 * n_cand_max, cand_rows_d + q0 * n_cand_max, out_scores_d + q0 * k,
                             out_rows_d + q0 * k, out_obj_d ? out_obj_d + q0 * k : nullptr, (int*)ws + 2 * q0,
                             (float*)(ws + p.norm), ws + p.flag, (uint32_t*)(ws + p.bits), (float*)(ws + p.gram), st) != 0)
      return api_fail(RFX_EUNSUPPORTED, "deep mmr select launch rejected (dim=%d dtype=%d)", ix.dim, ix.dtype);
  }
  const hipError_t e2 = hipGetLastError();
  if (e2 != hipSuccess) return api_fail(RFX_EDEVICE, "deep mmr select: %s", hipGetErrorString(e2));
  return RFX_OK;
}

}  // extern "C"
