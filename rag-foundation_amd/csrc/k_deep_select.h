// k_deep_select.h — the selection every deep search ends in: each question's k best candidate keys (k_cand_keys.h)
// out of a slab of them, and the order of a question's re-scored candidates.  Callers: the IVF deep search
// (ivf_api.hip), the sampled-threshold search (k_deep_sampled.hip) and the lexical deep search (lex_api.hip).
// Design: DESIGN §4.19.
//
// deep_select_kernel: one workgroup of 1,024 threads per question.  Most-significant-first radix passes of 8 bits
// over the key (256-bin histogram, suffix scan, the bin of the k-th key extends the prefix) until the keys above
// the prefix and in its bin number at most 2 * KB; those are gathered into LDS, sorted (bitonic, 2 * KB keys)
// and the k best written.  The output score is decoded from the key, so a -0.0 score is reported as +0.0.
// deep_order_kernel: the same sort over the re-ranked candidates of a question.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "deep_plan.h"

namespace rfx {

// slab: question q's keys at [q * qcap, q * qcap + n_keys[q]) (0 = none; qcap even, slab 16-B aligned: the
// selection reads 16 B).  Each question's k best keys (65 <= k <= 1,024) -> out_s / out_r [nq][k], padded (-inf, -1)
int launch_deep_select(const uint64_t* slab, int64_t qcap, const int* n_keys, int64_t nq, int k, float* out_s,
                       int64_t* out_r, hipStream_t st);
// s / r [nq][n] (n <= 1,024; r < 0 or a NaN score: no candidate) -> the k <= n best by (score desc, row asc)
int launch_deep_order(const float* s, const int64_t* r, int64_t nq, int n, int k, float* out_s, int64_t* out_r,
                      hipStream_t st);

}  // namespace rfx
