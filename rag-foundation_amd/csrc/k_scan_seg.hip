// k_scan_seg.hip — launcher of the segmented scan (kernel template: k_scan_seg.h, instantiated in
// seg_<dtype>.hip) and the fill of its candidate buffer.
//
// Path: questions under different metadata filters in one launch (gemini_rag.py:463-469's metadata_filter,
// validated at chat.py:295-335); the final answer is launch_topk_merge_lists' (k_scan_valu.hip).
#include "k_scan_seg.h"

namespace rfx {

// Every candidate slot starts as the project's empty slot (-inf, kEmptyRow): a group cut into fewer chunks
// than the call's lists per query, or a group without rows, leaves lists nobody writes.
__global__ __launch_bounds__(256) void seg_fill_kernel(float* __restrict__ cs, int* __restrict__ cr, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    cs[i] = -__builtin_inff();
    cr[i] = kEmptyRow;
  }
}

int seg_k_slot(int k) { return k <= 16 ? 16 : 64; }

bool seg_supported(int D, int dtype) {
  const int esz = dtype == RFX_F32 ? 4 : 2;
  const int vpl = (D * esz / 16 + 15) / 16;
  // 8 widened queries + the block merge's lists (16 KB at K = 64) within the 64 KB a launch gets by default
  return D > 0 && D % 64 == 0 && vpl <= 16 && (size_t)kSegSlice * D * sizeof(float) + 16384 <= 65536;
}

int launch_scan_seg(const void* X, int nrows, int D, int dtype, const void* Q, int64_t nq, int k,
                    const SegItemDev* items, int n_items, const SegRangeDev* R, float* cs, int* cr, int n_lists,
                    hipStream_t st) {
  if (!seg_supported(D, dtype) || k < 1 || k > 64) return -1;
  const int k_slot = seg_k_slot(k);
  const int64_t n = nq * n_lists * k_slot;
  if (n > 0) {
    const int blocks = (int)std::min<int64_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(seg_fill_kernel, dim3(blocks), dim3(256), 0, st, cs, cr, n);
  }
  if (n_items <= 0) return 0;
  const int esz = dtype == RFX_F32 ? 4 : 2;
  const int vpl = (D * esz / 16 + 15) / 16;
  const size_t lds = (size_t)kSegSlice * D * sizeof(float);
  const uint8_t* Xb = (const uint8_t*)X;
  if (dtype == RFX_F32) return launch_seg_f32(k_slot, vpl, n_items, lds, st, Xb, nrows, D, Q, items, R, cs, cr, n_lists);
  if (dtype == RFX_BF16) return launch_seg_bf16(k_slot, vpl, n_items, lds, st, Xb, nrows, D, Q, items, R, cs, cr, n_lists);
  return launch_seg_f16(k_slot, vpl, n_items, lds, st, Xb, nrows, D, Q, items, R, cs, cr, n_lists);
}

}  // namespace rfx
