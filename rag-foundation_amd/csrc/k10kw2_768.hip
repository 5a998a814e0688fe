// k10kw2_768.hip — instantiation unit of the wide form of the int8 screen kernel (k_scan_screen.h: top-k 11..64,
// lists of 16; plan 12), 2-wave (batches of 9..64 questions), d 768.
#include "k_scan_screen.h"

namespace rfx {
namespace k10 {
RFX_K10_INSTANTIATE_WIDE(768, 2, w2_ring<768>(), w2_mode<768>(), launch_768_wide_w2)
}  // namespace k10
}  // namespace rfx
