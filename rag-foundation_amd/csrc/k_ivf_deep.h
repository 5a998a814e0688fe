// k_ivf_deep.h — IVF deep search: the top-k of the probed posting lists for k in 65..1,024 (rfx_ivf_search_deep).
// Numerics: oracle/ivf.py, as the list scan of k_ivf_scan.hip; design: DESIGN §4.19.
//
// An IVF question ranks the rows of its probed lists only, a bounded and known count, so every probed row's
// score is written once and each question's k best are selected afterwards: two kernels, nothing in the scan
// waits on a sort.
//
// A candidate is one u64 key, as in k_deep.h: (ord_f32(score + 0.0f) << 32) | ~row.  A larger key is a better
// candidate under (score desc, row asc); key 0 is "none" (an ineligible row).  The output score is decoded from
// the key, so a -0.0 score is reported as +0.0.
//
// Slab: question q owns slab[q * qcap, (q + 1) * qcap).  Its probe slot j (pair p = q * nprobe + j) owns the
// run [pair_base[p], pair_base[p] + rows of the probed list), pair_base the exclusive prefix of the probed
// lists' lengths in slot order, n_keys[q] their total (pair_base_kernel).  qcap >= the rows of the nprobe
// longest lists >= n_keys[q], and is even (the selection reads 16 B).
//
// list_score_kernel<NC, E>: list_scan_kernel's decomposition (block (list, split), a wave's 64-row chunk one lane
// per row, chunk-major 16-B loads in double-buffered groups of 4, the list's pairs in batches of 8, questions
// through scalar loads into v_dot4) without the top-k lists: per staged pair the lane stores its row's key, a
// wave's store one 512-B run.
//
// deep_select_kernel: one workgroup of 1,024 threads per question.  Most-significant-first radix passes of 8 bits
// over the key (256-bin histogram, suffix scan, the bin of the k-th key extends the prefix) until the keys above
// the prefix and in its bin number at most 2 * KB; those are gathered into LDS, sorted (bitonic, 2 * KB keys)
// and the k best written.  deep_order_kernel: the same sort over the re-ranked candidates of a question.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "deep_plan.h"

namespace rfx {
namespace ivf {

constexpr int kDeepMaxProbe = 64;  // the C ABI's nprobe limit

// top[j] = the rows of the j longest lists, j = 0..64 (host; off = the nlist + 1 list offsets)
inline void deep_top_lists(const int64_t* off, int nlist, int64_t (&top)[kDeepMaxProbe + 1]) {
  std::vector<int64_t> len((size_t)nlist);
  for (int i = 0; i < nlist; ++i) len[i] = off[i + 1] - off[i];
  const int m = std::min(nlist, kDeepMaxProbe);
  std::partial_sort(len.begin(), len.begin() + m, len.end(), std::greater<int64_t>());
  top[0] = 0;
  for (int j = 1; j <= kDeepMaxProbe; ++j) top[j] = top[j - 1] + (j <= m ? len[j - 1] : 0);
}

// The slab stride of a question: the rows of the nprobe longest lists at the last build, plus the rows added
// since (wherever they went, no nprobe lists hold more), at most every row; even, at least 2.
inline int64_t deep_qcap(const int64_t (&top)[kDeepMaxProbe + 1], int nprobe, int64_t rows, int64_t built_rows) {
  const int64_t raw = std::min(rows, top[nprobe] + (rows - built_rows));
  return (std::max<int64_t>(raw, 1) + 1) & ~(int64_t)1;
}

// pid [nq][nprobe]: the probed lists -> pair_base [nq][nprobe], n_keys [nq]
void launch_pair_base(const int64_t* pid, const int64_t* off, int64_t nq, int nprobe, int* pair_base, int* n_keys,
                      hipStream_t st);
// every probed row's key into the slab; row_mask == nullptr: every row eligible.  -1: no kernel for D.
int launch_list_score(int D, int m, int splits, const int8_t* codes, const float* inv, const int* ids, const int64_t* off,
                      const int* pair_off, const int* pairs, int nprobe, const int8_t* qq, const float* qinv,
                      const int* pair_base, int64_t qcap, uint64_t* slab, const uint32_t* row_mask, hipStream_t st);
// each question's k best keys (65 <= k <= 1,024) -> out_s / out_r [nq][k], padded (-inf, -1)
int launch_deep_select(const uint64_t* slab, int64_t qcap, const int* n_keys, int64_t nq, int k, float* out_s,
                       int64_t* out_r, hipStream_t st);
// s / r [nq][n] (n <= 1,024; r < 0 or a NaN score: no candidate) -> the k <= n best by (score desc, row asc)
int launch_deep_order(const float* s, const int64_t* r, int64_t nq, int n, int k, float* out_s, int64_t* out_r,
                      hipStream_t st);

}  // namespace ivf
}  // namespace rfx
