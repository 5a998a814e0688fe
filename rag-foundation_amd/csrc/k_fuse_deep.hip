// k_fuse_deep.hip — the deep rank-fusion kernel and its launcher (see k_fuse_deep.h).
#include "k_fuse_deep.h"

#include "k_fuse.h"
#include "rfx_device.h"

namespace rfx {
namespace {

constexpr int kFdThreads = 256;
constexpr int kFdWaves = kFdThreads / kWave;
constexpr int kFdSlots = 4096;                    // twice the distinct rows two full lists can hold
constexpr int kFdMaxCand = 2 * kFuseDeepMaxList;  // distinct rows at most
constexpr unsigned long long kFdEmpty = ~0ull;    // no row id is negative
constexpr int kFdAbsent = 0x7fffffff;
constexpr size_t kFdLds = (size_t)kFdSlots * 16 + (size_t)kFdMaxCand * 16;  // 96 KB

__device__ __forceinline__ int fd_home(unsigned long long row) {
  return (int)((row * 0x9E3779B97F4A7C15ull) >> 52);  // the top 12 bits: a slot in [0, 4096)
}

// One list into the table: ranks in list order (every valid entry advances the rank), a row keeps its first.
// 256 entries per trip; the trip count is uniform.
__device__ __forceinline__ void fd_insert_list(const int64_t* __restrict__ list, int n, unsigned long long* hkey,
                                               int* hrank, int* s_wave) {
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  int base = 0;
  for (int c0 = 0; c0 < n; c0 += kFdThreads) {
    long long row = -1;
    if (c0 + tid < n) row = list[c0 + tid];
    const bool valid = row >= 0;
    const uint64_t m = __ballot(valid);
    if (lane == 0) s_wave[w] = __popcll(m);
    __syncthreads();
    int before = base, total = 0;
#pragma unroll
    for (int ww = 0; ww < kFdWaves; ++ww) {
      const int c = s_wave[ww];
      if (ww < w) before += c;
      total += c;
    }
    if (valid) {
      const int rank = 1 + before + __popcll(m & below);
      int s = fd_home((unsigned long long)row);
      for (;;) {  // linear probing; the table is never more than half full
        const unsigned long long prev = atomicCAS(&hkey[s], kFdEmpty, (unsigned long long)row);
        if (prev == kFdEmpty || prev == (unsigned long long)row) break;
        s = (s + 1) & (kFdSlots - 1);
      }
      atomicMin(&hrank[s], rank);
    }
    base += total;
    __syncthreads();  // s_wave is written again
  }
}

// a is ranked before b: f desc (f >= 0: its bits order as an integer), then row asc; padding (0, ~0) is last
__device__ __forceinline__ bool fd_before(unsigned long long fa, unsigned long long ra, unsigned long long fb,
                                          unsigned long long rb) {
  return fa > fb || (fa == fb && ra < rb);
}

__global__ __launch_bounds__(kFdThreads) void rrf_fuse_deep_kernel(
    const int64_t* __restrict__ dense_r, int n_dense_max, const int64_t* __restrict__ lex_r, int n_lex_max, int k,
    const float* __restrict__ alpha, const int32_t* __restrict__ nd_t, const int32_t* __restrict__ nl_t, int rrf_c,
    float* __restrict__ out_s, int64_t* __restrict__ out_r, int32_t* __restrict__ out_ranks) {
  extern __shared__ __attribute__((aligned(16))) uint8_t fd_lds[];
  unsigned long long* hkey = (unsigned long long*)fd_lds;   // [slots] row id, kFdEmpty = free
  int* hrd = (int*)(fd_lds + (size_t)kFdSlots * 8);         // [slots] first dense rank, kFdAbsent = none
  int* hrl = hrd + kFdSlots;                                // [slots] first lexical rank
  unsigned long long* sf = (unsigned long long*)(fd_lds + (size_t)kFdSlots * 16);  // [cand] bits of f
  unsigned long long* sr = sf + kFdMaxCand;                 // [cand] row
  __shared__ int s_wave[kFdWaves];
  __shared__ int s_cnt;
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  const int nd = min(max(nd_t[q], 0), min(n_dense_max, kFuseDeepMaxList));
  const int nl = min(max(nl_t[q], 0), min(n_lex_max, kFuseDeepMaxList));
  const double A = (double)alpha[q];
  const double c = (double)rrf_c;

  for (int s = tid; s < kFdSlots; s += kFdThreads) hkey[s] = kFdEmpty, hrd[s] = kFdAbsent, hrl[s] = kFdAbsent;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  fd_insert_list(dense_r + q * n_dense_max, nd, hkey, hrd, s_wave);
  fd_insert_list(lex_r + q * n_lex_max, nl, hkey, hrl, s_wave);
  __syncthreads();
  // every occupied slot is one distinct row: its score, into the sort buffer in any order
  for (int s = tid; s < kFdSlots; s += kFdThreads) {
    const unsigned long long row = hkey[s];
    if (row == kFdEmpty) continue;
    const int rd = hrd[s] == kFdAbsent ? 0 : hrd[s], rl = hrl[s] == kFdAbsent ? 0 : hrl[s];
    const double f = rrf_score(A, c, rd, rl);
    const int pos = atomicAdd(&s_cnt, 1);
    if (pos < kFdMaxCand) sf[pos] = (unsigned long long)__double_as_longlong(f), sr[pos] = row;
  }
  __syncthreads();
  const int total = min(s_cnt, kFdMaxCand);
  int ns = 2;
  while (ns < total) ns <<= 1;
  for (int i = total + tid; i < ns; i += kFdThreads) sf[i] = 0ull, sr[i] = kFdEmpty;
  __syncthreads();
  for (int k2 = 2; k2 <= ns; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < ns / 2; i += kFdThreads) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
        const unsigned long long fa = sf[lo], ra = sr[lo], fb = sf[hi], rb = sr[hi];
        if (fd_before(fb, rb, fa, ra) == ((lo & k2) == 0)) {
          sf[lo] = fb, sr[lo] = rb;
          sf[hi] = fa, sr[hi] = ra;
        }
      }
      __syncthreads();
    }
  for (int j = tid; j < k; j += kFdThreads) {
    const int64_t o = q * k + j;
    if (j < total) {
      const unsigned long long row = sr[j];
      out_s[o] = (float)__longlong_as_double((long long)sf[j]);
      out_r[o] = (int64_t)row;
      if (out_ranks) {
        int s = fd_home(row);
        while (hkey[s] != row) s = (s + 1) & (kFdSlots - 1);  // the row is in the table
        out_ranks[o * 2] = hrd[s] == kFdAbsent ? 0 : hrd[s];
        out_ranks[o * 2 + 1] = hrl[s] == kFdAbsent ? 0 : hrl[s];
      }
    } else {
      out_s[o] = -__builtin_inff();
      out_r[o] = -1;
      if (out_ranks) out_ranks[o * 2] = 0, out_ranks[o * 2 + 1] = 0;
    }
  }
}

}  // namespace

int launch_rrf_fuse_deep(const int64_t* dense_r, int n_dense_max, const int64_t* lex_r, int n_lex_max, int64_t nq, int k,
                         const float* alpha_d, const int32_t* nd_d, const int32_t* nl_d, int rrf_c, float* out_s,
                         int64_t* out_r, int32_t* out_ranks, hipStream_t st) {
  if (nq < 1 || nq > 1024 || k < 1 || k > kFuseDeepMaxList || n_dense_max < 1 || n_dense_max > kFuseDeepMaxList ||
      n_lex_max < 1 || n_lex_max > kFuseDeepMaxList || rrf_c < 1)
    return -1;
  if (!dense_r || !lex_r || !alpha_d || !nd_d || !nl_d || !out_s || !out_r) return -1;
  auto kern = rrf_fuse_deep_kernel;
  if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFdLds) != hipSuccess)
    return -1;
  hipLaunchKernelGGL(kern, dim3((unsigned)nq), dim3(kFdThreads), kFdLds, st, dense_r, n_dense_max, lex_r, n_lex_max, k,
                     alpha_d, nd_d, nl_d, rrf_c, out_s, out_r, out_ranks);
  return 0;
}

}  // namespace rfx
