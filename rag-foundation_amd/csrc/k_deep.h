// k_deep.h — deep search: the exact top-k of a flat bf16 / f16 store for k in 65..1,024 (rfx_search_deep).
// Host plan: deep_plan.h; design and LDS budget: DESIGN §4.18.
//
// Path: the retrieval slice of ask_stream (gemini_rag.py:517-551) at the depth a re-ranker, rank fusion or a
// recall@100 evaluation reads.  The per-lane / per-wave sorted lists of the other scans (4..64 entries in
// registers) do not reach a thousand entries; selection here is a threshold, a buffer and a periodic sort,
// all in LDS.
//
// A candidate is one u64 key, cand_key of k_cand_keys.h: a larger key is a better candidate under the ranking
// rule (score desc, row asc), so one integer compare carries the tie-break through every step; key 0 is "no
// candidate".
//
// deep_scan_kernel: grid (ranges, question groups), 256 threads.  The group's questions (16, or 8 at KB
// 1,024) stay in registers as the B fragments of v_mfma_f32_16x16x32; each wave streams 16-row tiles of the
// range as A fragments straight from global memory (two 16-B loads per lane and 64 columns, so a wave
// instruction pair reads whole 128-B lines), the next tile's loads in flight under the current tile's MFMAs.
// A lane holds 4 rows of one question: it compares them with its question's threshold (a register) and the
// wave ballots once; only a tile with a passing row touches LDS (slots claimed by cand_claim: ballot + prefix
// count, one LDS add per question and accumulator register).  Every check_rounds rounds the workgroup meets: a
// buffer that could overflow before the next meeting is cut (cand_cut: bitonic sort in place of 2 * KB keys, its
// KB best stay and the KB-th becomes the threshold).  Rows of a range arrive in ascending order between
// meetings, so a score EQUAL to the threshold's is a worse key and is dropped by the score compare alone.
//
// deep_merge_kernel: one workgroup per question streams the ranges' lists through the same buffer routines
// (full-key compare against the threshold), sorts, re-scores the k best by the score rule of every search
// (fl32 of the f64 dot of the stored values), sorts again and writes k (score, int64 row), then (-inf, -1).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "deep_plan.h"

namespace rfx {

// ws: [nq][p.ranges][p.kb] u64 keys (deep_ws_bytes).  mask: optional row bitmap (rfx_search_masked's form).
// Returns 0, or -1 for arguments no kernel serves (nothing launched).
// nq_dev (optional, device): the questions to answer are the first min(nq, *nq_dev), a count that only the device
// knows when the call is enqueued (the fallback of k_deep_sampled.h); the grid is nq's, groups past the count exit.
int launch_deep_search(const DeepPlan& p, const void* X, int64_t nrows, int D, int dtype, const void* Q, int64_t nq, int k,
                       const uint32_t* mask, uint64_t* ws, float* out_s, int64_t* out_r, hipStream_t st,
                       const int* nq_dev = nullptr);

// The merge alone, for a scan that filled ws itself (k_deep_f32.h): any dtype the score rule serves.
void launch_deep_merge(const DeepPlan& p, const void* X, int64_t nrows, int D, int dtype, const void* Q, int64_t nq, int k,
                       const uint64_t* ws, float* out_s, int64_t* out_r, hipStream_t st, const int* nq_dev = nullptr);

}  // namespace rfx
