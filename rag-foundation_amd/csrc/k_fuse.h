// k_fuse.h — reciprocal-rank fusion of a dense and a lexical candidate list (rfx_lex_fuse).
//
// Path: after the retrieval slice of ask_stream (gemini_rag.py:517-551) has run twice (dense, BM25): each
// distinct row of the two lists scores f = A / (c + rank_d) + (1 - A) / (c + rank_l) in f64, every operation
// rounded on its own (a list the row is absent from contributes 0.0); the k best by (f desc, row asc).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rfx {

constexpr int kFuseMaxList = 64;

// One wave per question.  dense_r / lex_r: [nq][n_dense_max] / [nq][n_lex_max] rows (< 0 = padding), of which
// the first nd[q] / nl[q] entries are used; alpha [nq] f32.  out_s / out_r [nq][k]; out_ranks (may be null)
// [nq][k][2] = {rank_d, rank_l}, 0 = absent.  Padding (-inf, -1, 0, 0).
int launch_rrf_fuse(const int64_t* dense_r, int n_dense_max, const int64_t* lex_r, int n_lex_max, int64_t nq, int k,
                    const float* alpha_d, const int32_t* nd_d, const int32_t* nl_d, int rrf_c, float* out_s,
                    int64_t* out_r, int32_t* out_ranks, hipStream_t st);

}  // namespace rfx
