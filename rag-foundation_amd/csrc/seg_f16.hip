// seg_f16.hip — instantiation unit of the segmented scan (k_scan_seg.h) for f16 indices.
#include "k_scan_seg.h"

namespace rfx {
int launch_seg_f16(int k_slot, int vpl, int n_items, size_t lds, hipStream_t st, const uint8_t* X, int nrows, int D,
                  const void* Q, const SegItemDev* items, const SegRangeDev* R, float* cs, int* cr, int n_lists) {
  return launch_seg_dt<RFX_F16>(k_slot, vpl, n_items, lds, st, X, nrows, D, Q, items, R, cs, cr, n_lists);
}
}  // namespace rfx
