// k_mmr.h — diversified retrieval: greedy MMR (maximal marginal relevance) selection over the top candidates
// of an ordinary search.
//
// Path: the stage after the retrieval slice of ask_stream (gemini_rag.py:517-551): the reference hands the k
// best chunks to the answer step as they come; overlapping chunk windows and re-uploaded files make them
// near-copies of each other.  Here k of n_cand >= k candidates are picked greedily, each pick trading its
// score against its similarity to what is already picked.
//
// One workgroup (4 waves) per query; every query has its own lambda and its own n_cand.
//   1. The candidates' rows are gathered by row id (16-byte loads) and checked for NaN (a tombstoned row is
//      padding).  bf16 / f16 rows are staged in LDS ([n_cand][D + 32] elements: the 64-byte pad spreads the
//      rows of one ds_read_b128 lane group over all banks); f32 rows do not fit and are read in place (they
//      stay in L2: 64 rows are 256 KB at most).
//   2. Greedy steps.  A similarity sim(i, j) is only ever used with j SELECTED, so the kernel never builds
//      the n_cand x n_cand matrix: after each pick j it computes the one column sim(., j) — (k - 1) * n_cand
//      dots instead of n_cand * (n_cand - 1) / 2 — with the f64 VALU: row j widened to f64 in LDS once, then
//      256 / pow2(n_cand) lanes per candidate, each an f64 FMA chain over 8-element pieces, summed by a xor
//      butterfly.  fl32 of that sum is the similarity (the score rule of every search, applied to two rows).
//      Wave 0 keeps one candidate per lane: m_i = max similarity to the picked, the objective in f64 with
//      every operation rounded on its own, a wave max, and the lowest lane among the equals.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rfx {

constexpr int kMmrThreads = 256;
constexpr int kMmrMaxCand = 64;
constexpr int kMmrMaxNq = 1024;
constexpr int kMmrRowPad = 32;                // elements of padding after a staged 16-bit row (64 bytes)
constexpr size_t kMmrLdsBudget = 158 * 1024;  // of the CU's 160 KB; the kernel's static arrays take about 1 KB

// Dynamic LDS of a launch: row j in f64, plus the staged rows when they fit (*staged).
size_t mmr_lds_bytes(int D, int dtype, int n_cand_max, bool* staged);

// lam_d [nq] f32 in [0, 1], ncand_d [nq] in 1..n_cand_max (clamped in the kernel), cand_s / cand_r
// [nq][n_cand_max], out_s / out_r / out_obj (may be null) [nq][k].  X: [nrows][D] of dtype; a candidate row
// outside [0, nrows) is padding.  Returns 0, or -1 for arguments it refuses (nothing launched).
int launch_mmr_select(const void* X, int64_t nrows, int D, int dtype, int64_t nq, int n_cand_max, int k,
                      const float* lam_d, const int* ncand_d, const float* cand_s, const int64_t* cand_r, float* out_s,
                      int64_t* out_r, float* out_obj, hipStream_t st);

}  // namespace rfx
