// k10k_768.hip — instantiation unit of the wide form of the int8 screen kernel (k_scan_screen.h: top-k 11..64,
// lists of 16; plan 12), 8-wave (batches of more than 64 questions), d 768.
#include "k_scan_screen.h"

namespace rfx {
namespace k10 {
RFX_K10_INSTANTIATE_WIDE(768, 8, kProdRing, kProdMode, launch_768_wide)
}  // namespace k10
}  // namespace rfx
