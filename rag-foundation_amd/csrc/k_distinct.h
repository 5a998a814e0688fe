// k_distinct.h — distinct-document search: collapse a sorted candidate list by document.
//
// Path: the retrieval slice of ask_stream (gemini_rag.py:517-551).  The reference's file-search tool answers
// with documents; every rfx_search* ranks rows, and a row is a chunk, so one long report fills all k places
// with its own chunk windows.  The rule: of the full ranking of the selected live rows (score desc, row asc)
// keep a row when no earlier row belongs to the same document; the answer is the first k kept rows.
//
// The kernel is the collapse of ONE sorted list of at most 64 candidates (the answer of any rfx_search* at
// k = n_cand); the exact search over the whole store is rounds of it (rfx.index.DeviceIndex.search_distinct).
// One wave per question, 4 questions per 256-thread block; lane i holds candidate i.
//   1. valid = the row is inside [0, rows); its document = row_doc[row] (-1: no live document).
//   2. A lane drops out when its document is < 0, when a lower lane holds the same document (a wave-uniform
//      loop of 64 shuffles), or when the document is among the have[q] documents already in out_docs[q].
//   3. A survivor's place is have[q] + the survivors below it (ballot, popcount under the lane mask); places
//      below k are written, places from the new count to k - 1 are padded (-inf, -1, -1), places below
//      have[q] are not touched.
//   4. out_n[q] = the new count; out_done[q] = the count reached k, or the list held fewer than n_cand valid
//      entries (the search ran out of rows: nothing is left to find).
// No LDS, no atomics; every lane of a wave runs every shuffle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rfx {

constexpr int kDistinctThreads = 256;
constexpr int kDistinctMaxCand = 64;
constexpr int kDistinctMaxNq = 1024;

// row_doc [rows] int32; cand_s / cand_r [nq][n_cand]; have (may be null: 0) [nq] in 0..k; out_s / out_r /
// out_docs [nq][k]; out_n / out_done [nq].  Returns 0, or -1 for arguments it refuses (nothing launched).
int launch_distinct_collapse(const int32_t* row_doc, int64_t rows, int nq, int n_cand, int k, const float* cand_s,
                             const int64_t* cand_r, const int32_t* have, float* out_s, int64_t* out_r,
                             int32_t* out_docs, int32_t* out_n, int32_t* out_done, hipStream_t st);

}  // namespace rfx
