// k_fuse.hip — the rank-fusion kernel and its launcher (see k_fuse.h).
#include "k_fuse.h"

#include "rfx_device.h"

namespace rfx {
namespace {

// f = A / (c + rank_d) + (1 - A) / (c + rank_l): IEEE f64 divisions, no contraction; rank 0 = absent = 0.0
__device__ __forceinline__ double rrf_score(double A, double c, int rank_d, int rank_l) {
#pragma clang fp contract(off)
  double fd = 0.0, fl = 0.0;
  if (rank_d > 0) {
    const double den = c + (double)rank_d;
    fd = A / den;
  }
  if (rank_l > 0) {
    const double oma = 1.0 - A;
    const double den = c + (double)rank_l;
    fl = oma / den;
  }
  return fd + fl;
}

// Lane i owns dense entry i and lexical entry i.  Candidates: slot i = dense entry i (with its lexical rank when
// the row is in both lists), slot 64 + i = lexical entry i when its row is NOT in the dense list.  A candidate's
// output position is the number of candidates that beat it (rows are distinct, so the order is total).
__global__ __launch_bounds__(kWave) void rrf_fuse_kernel(const int64_t* __restrict__ dense_r, int n_dense_max,
                                                         const int64_t* __restrict__ lex_r, int n_lex_max, int k,
                                                         const float* __restrict__ alpha,
                                                         const int32_t* __restrict__ nd_t,
                                                         const int32_t* __restrict__ nl_t, int rrf_c,
                                                         float* __restrict__ out_s, int64_t* __restrict__ out_r,
                                                         int32_t* __restrict__ out_ranks) {
  __shared__ long long s_dr[kFuseMaxList], s_lr[kFuseMaxList];  // rows, -1 = padding
  __shared__ int s_drank[kFuseMaxList], s_lrank[kFuseMaxList];
  __shared__ double s_f[2 * kFuseMaxList];
  __shared__ long long s_row[2 * kFuseMaxList];  // -1 = no candidate in the slot
  const int lane = threadIdx.x;
  const int64_t q = blockIdx.x;
  const int nd = min(max(nd_t[q], 0), min(n_dense_max, kFuseMaxList));
  const int nl = min(max(nl_t[q], 0), min(n_lex_max, kFuseMaxList));
  const double A = (double)alpha[q];
  const double c = (double)rrf_c;

  long long dr = -1, lr = -1;
  if (lane < nd) dr = dense_r[q * n_dense_max + lane];
  if (lane < nl) lr = lex_r[q * n_lex_max + lane];
  if (dr < 0) dr = -1;
  if (lr < 0) lr = -1;
  // rank = 1 + the valid entries before it
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  const int drank = dr >= 0 ? 1 + __popcll(__ballot(dr >= 0) & below) : 0;
  const int lrank = lr >= 0 ? 1 + __popcll(__ballot(lr >= 0) & below) : 0;
  s_dr[lane] = dr, s_lr[lane] = lr, s_drank[lane] = drank, s_lrank[lane] = lrank;
  __syncthreads();
  // a row repeated inside one list counts at its first (best) position only
  int my_l = 0;       // the dense entry's lexical rank
  bool dup_d = false, in_dense = false, dup_l = false;
  for (int j = 0; j < kFuseMaxList; ++j) {  // broadcast reads
    const long long rj_d = s_dr[j], rj_l = s_lr[j];
    if (dr >= 0 && rj_l == dr && my_l == 0) my_l = s_lrank[j];
    if (dr >= 0 && j < lane && rj_d == dr) dup_d = true;
    if (lr >= 0 && rj_d == lr) in_dense = true;
    if (lr >= 0 && j < lane && rj_l == lr) dup_l = true;
  }
  const bool cand_a = dr >= 0 && !dup_d;
  const bool cand_b = lr >= 0 && !in_dense && !dup_l;
  const double fa = rrf_score(A, c, drank, my_l);
  const double fb = rrf_score(A, c, 0, lrank);
  s_f[lane] = fa, s_row[lane] = cand_a ? dr : -1;
  s_f[kFuseMaxList + lane] = fb, s_row[kFuseMaxList + lane] = cand_b ? lr : -1;
  __syncthreads();
  int pos_a = 0, pos_b = 0;
  const int total = __popcll(__ballot(cand_a)) + __popcll(__ballot(cand_b));
  for (int j = 0; j < 2 * kFuseMaxList; ++j) {
    const long long rj = s_row[j];
    if (rj < 0) continue;  // wave-uniform
    const double fj = s_f[j];
    pos_a += fj > fa || (fj == fa && rj < dr);
    pos_b += fj > fb || (fj == fb && rj < lr);
  }
  if (cand_a && pos_a < k) {
    out_s[q * k + pos_a] = (float)fa;
    out_r[q * k + pos_a] = dr;
    if (out_ranks) out_ranks[(q * k + pos_a) * 2] = drank, out_ranks[(q * k + pos_a) * 2 + 1] = my_l;
  }
  if (cand_b && pos_b < k) {
    out_s[q * k + pos_b] = (float)fb;
    out_r[q * k + pos_b] = lr;
    if (out_ranks) out_ranks[(q * k + pos_b) * 2] = 0, out_ranks[(q * k + pos_b) * 2 + 1] = lrank;
  }
  for (int e = total + lane; e < k; e += kWave) {
    out_s[q * k + e] = -__builtin_inff();
    out_r[q * k + e] = -1;
    if (out_ranks) out_ranks[(q * k + e) * 2] = 0, out_ranks[(q * k + e) * 2 + 1] = 0;
  }
}

}  // namespace

int launch_rrf_fuse(const int64_t* dense_r, int n_dense_max, const int64_t* lex_r, int n_lex_max, int64_t nq, int k,
                    const float* alpha_d, const int32_t* nd_d, const int32_t* nl_d, int rrf_c, float* out_s,
                    int64_t* out_r, int32_t* out_ranks, hipStream_t st) {
  if (nq < 1 || nq > 1024 || k < 1 || k > kFuseMaxList || n_dense_max < 1 || n_dense_max > kFuseMaxList ||
      n_lex_max < 1 || n_lex_max > kFuseMaxList || rrf_c < 1)
    return -1;
  if (!dense_r || !lex_r || !alpha_d || !nd_d || !nl_d || !out_s || !out_r) return -1;
  hipLaunchKernelGGL(rrf_fuse_kernel, dim3((unsigned)nq), dim3(kWave), 0, st, dense_r, n_dense_max, lex_r, n_lex_max, k,
                     alpha_d, nd_d, nl_d, rrf_c, out_s, out_r, out_ranks);
  return 0;
}

}  // namespace rfx
