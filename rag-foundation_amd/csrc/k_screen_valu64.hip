// k_screen_valu64.hip — kernel 11 with A-lists of 64 (17 <= k <= 64): the instantiations of
// k_screen_valu.hip's kernel template at list length 64 and their launcher (launch_screen_valu64), in a
// translation unit of their own so that the two list lengths compile in parallel.
#define RFX_K11_LIST 64
#include "k_screen_valu.hip"
