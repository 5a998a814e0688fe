// k_fuse_deep.h — reciprocal-rank fusion of a dense and a lexical candidate list of up to 1,024 entries each
// (rfx_lex_fuse_deep; rule: k_fuse.h / DESIGN §4.14, design: DESIGN §4.21).
//
// rrf_fuse_deep_kernel: one workgroup of 256 threads per question.  An entry's rank is 1 + the valid entries before
// it (ballot + popcount per wave, wave offsets through LDS).  Rows are matched in an LDS hash table of 4,096 slots
// on the row id (64-bit compare-and-swap claims a slot, atomicMin keeps a row's first rank in either list), each
// occupied slot scores f in f64 as rrf_fuse_kernel does, and the up to 2,048 (f bits, row) pairs are sorted in LDS
// (bitonic; f >= 0, so its bit pattern orders as an integer) by (f desc, row asc).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rfx {

constexpr int kFuseDeepMaxList = 1024;

// dense_r / lex_r: [nq][n_dense_max] / [nq][n_lex_max] rows (< 0 = padding), of which the first nd[q] / nl[q]
// entries are used; alpha [nq] f32.  out_s / out_r [nq][k]; out_ranks (may be null) [nq][k][2] = {rank_d, rank_l},
// 0 = absent.  Padding (-inf, -1, 0, 0).  -1: arguments outside the kernel's range.
int launch_rrf_fuse_deep(const int64_t* dense_r, int n_dense_max, const int64_t* lex_r, int n_lex_max, int64_t nq, int k,
                         const float* alpha_d, const int32_t* nd_d, const int32_t* nl_d, int rrf_c, float* out_s,
                         int64_t* out_r, int32_t* out_ranks, hipStream_t st);

}  // namespace rfx
