// k_mmr_deep.h — diversified retrieval at depth: the MMR rule of DESIGN §4.13 (k_mmr.h) over 65..1,024
// candidates per question, k up to the candidate count.  bf16 / f16 rows, dim % 64 == 0 up
// to 1,024.
//
// Path: the stage after the retrieval slice of ask_stream (gemini_rag.py:517-551) at the depth of the deep
// searches: the pool of a diversified answer (4k candidates for k >= 17) and the candidate set of a re-ranker.
//
// k_mmr.hip keeps a candidate per lane and the rows in LDS; 1,024 rows do not fit, and its column form would
// re-read them from L2 / HBM at every step.  Here a cheap matrix-core pass under a rigorous error bound does
// the bulk, and the exact f64 rule decides only where the bound cannot:
//   1. mmr_gram_kernel: per question the approximate similarity matrix G~ = C C^T of its gathered candidate
//      rows (v_mfma_f32_16x16x32, f32 accumulators).  Grid (upper-triangle tile pairs) x (questions); a
//      workgroup owns one 64 x 64 tile, gathers its two row panels by row id in 16-byte pieces (16 loads in
//      flight per thread) and stages them through LDS in slabs of 256 columns, in the XOR-swizzled 512-byte line
//      image of k_deep_sampled.hip (chunk c of row r at c ^ (r & 15): a fragment read is conflict-free).  A row
//      leaves L2 once per tile.  The tile and its mirror go to the question's [n_pad][n_pad] f32 matrix.  The
//      diagonal tiles also write, per candidate, a_i >= ||x_i||_2 (f64 sum of squares, rounded upward to f32)
//      and the padding flag (row out of range, or a NaN in the row), and every tile clears its part of the
//      question's bit matrix of exact pairs.
//   2. The bound.  Products of two bf16 / f16 values are exact in f32, so G~ errs by its additions only: for
//      any order and at most one ulp per addition, |G~_ij - fl32(sim_ij)| <= eps_ij = gamma a_i a_j +
//      D 2^-120, gamma = (2 D + 1) 2^-24.  A non-finite G~_ij or a_i leaves the pair undecided.  Nothing else
//      relies on how the matrix core rounds.
//   3. mmr_deep_select_kernel: one workgroup (4 waves) per question, candidate tid + 256 c in registers of
//      thread tid (score, m~ = max of G~ over the picked, its error e, availability).  After a pick j the step
//      reads row j of G~ (contiguous), updates m~ and e, brackets every objective by monotone rounding
//      [lo, hi], reduces B = max lo, and calls a candidate with hi + 1e-12 >= B a contender.  A wave per
//      contender then finds its exact m: only the picked j with G~_ij + eps_ij >= max_j' (G~_ij' - eps_ij') can
//      hold the maximum, and each of those gets the f64 FMA dot of the two rows read in place (one wave per dot),
//      written back over G~_ij and marked in the bit matrix, so no pair is scored twice.  The pick is the
//      contender with the largest exact objective, the lowest position among equals.  One contender and no
//      objective output asked for: no exact dot at all.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mmr_deep_plan.h"

namespace rfx {

constexpr int kMmrDeepThreads = 256;

// One slice of a call: questions [0, nq) of the pointers given (the caller has advanced them to the slice).
// lam_d / ncand_d [nq], cand_s / cand_r [nq][n_cand_max], out_* [nq][k] (out_obj may be null), stats [nq][2]
// (contenders summed over the steps, exact dots); norm [nq][n_pad] f32, flag [nq][n_pad] u8, bits
// [nq][n_pad][n_pad / 32] u32 and gram [nq][n_pad][n_pad] f32 are the slice's scratch.  Two launches on st.
// Returns 0, or -1 for arguments it refuses (nothing launched).
int launch_mmr_deep(const MmrDeepPlan& p, const void* X, int64_t nrows, int D, int dtype, int nq, int n_cand_max, int k,
                    const float* lam_d, const int* ncand_d, const float* cand_s, const int64_t* cand_r, float* out_s,
                    int64_t* out_r, float* out_obj, int* stats, float* norm, uint8_t* flag, uint32_t* bits, float* gram,
                    hipStream_t st);

}  // namespace rfx
