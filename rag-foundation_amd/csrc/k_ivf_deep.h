// k_ivf_deep.h — IVF deep search: the top-k of the probed posting lists for k in 65..1,024 (rfx_ivf_search_deep).
// Numerics: oracle/ivf.py, as the list scan of k_ivf_scan.hip; design: DESIGN §4.19.
//
// An IVF question ranks the rows of its probed lists only, a bounded and known count, so every probed row's
// score is written once and each question's k best are selected afterwards: two kernels, nothing in the scan
// waits on a sort.
//
// A candidate is one u64 key, cand_key of k_cand_keys.h; key 0 is an ineligible row.  The output score is decoded
// from the key, so a -0.0 score is reported as +0.0.
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
// The selection (each question's k best of its slab) and the order of the re-ranked candidates: k_deep_select.h.
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
}  // namespace ivf
}  // namespace rfx
