// k10kw2_1024.hip — instantiation unit of the wide form of the int8 screen kernel (k_scan_screen.h: top-k 11..64,
// lists of 16; plan 12), 2-wave (batches of 9..64 questions), d 1024.
#include "k_scan_screen.h"

namespace rfx {
namespace k10 {
RFX_K10_INSTANTIATE_WIDE(1024, 2, w2_ring<1024>(), w2_mode<1024>(), launch_1024_wide_w2)
}  // namespace k10
}  // namespace rfx
