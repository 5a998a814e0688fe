// k_deep_select.hip — the selection kernels of the deep searches (k_deep_select.h): a radix selection and an LDS
// sort per question.  gfx950 only.
#include "k_deep_select.h"

#include "k_cand_keys.h"

namespace rfx {
namespace {

constexpr int kSelThreads = 1024;  // deep_select_kernel / deep_order_kernel: 16 waves
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kSelMaxKeys = 2 * kDeepMaxK;  // the sort buffer: 2 * KB keys, 16 KiB at KB 1,024

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

// ---- the k largest of a question's keys ---------------------------------------------------------------------------
// Histogram: one private 256-bin table per wave (16 KiB), so LDS adds of different waves never meet, and one test
// in front of the adds: when every participating lane of the wave holds the same bin — the high passes, where the
// byte is the score's sign and exponent and nearly every key agrees — one lane adds the count.  Otherwise each lane
// adds 1 to its bin; in the low passes (mantissa and row bits) the bins are spread and such adds rarely collide.
// A ballot per distinct bin would serve the first case equally and take up to 64 rounds in the second.
__global__ __launch_bounds__(kSelThreads) void deep_select_kernel(const uint64_t* __restrict__ slab, int64_t qcap,
                                                                  const int* __restrict__ n_keys, int KB, int k,
                                                                  float* __restrict__ out_s, int64_t* __restrict__ out_r) {
  __shared__ uint32_t hist[kSelWaves][256];
  __shared__ __attribute__((aligned(16))) uint64_t buf[kSelMaxKeys];
  __shared__ uint32_t s_bin, s_above, s_inbin;
  __shared__ int s_cnt;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t q = blockIdx.x;
  const int n = n_keys[q], N2 = 2 * KB;
  const u64x2* kv = (const u64x2*)(slab + q * qcap);  // q * qcap is even: 16-B aligned
  const int nv = (n + 1) / 2;                         // (an odd n: the last pair's second key is masked by 2 i + 1 < n)

  uint64_t lo = 0, pmask = 0;  // the prefix found so far and its bits; a key takes part when (key & pmask) == lo
  uint32_t above = 0;          // keys above the prefix
  if (n > N2) {
    for (int pass = 0; pass < 8; ++pass) {
      const int shift = 56 - 8 * pass;
      for (int i = tid; i < kSelWaves * 256; i += kSelThreads) (&hist[0][0])[i] = 0;
      __syncthreads();
      for (int i0 = 0; i0 < nv; i0 += kSelThreads) {  // (uniform trip count: the ballots below)
        const int i = i0 + tid;
        u64x2 v = {0ull, 0ull};
        if (i < nv) v = pass == 0 ? __builtin_nontemporal_load(kv + i) : kv[i];  // read once, then from L2
        const uint64_t two[2] = {v.x, 2 * i + 1 < n ? v.y : 0ull};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const uint64_t key = two[h];
          const bool part = key != 0 && (key & pmask) == lo;
          const int bin = (int)(key >> shift) & 255;
          const uint64_t act = __ballot(part);
          if (act) {
            const int first = __builtin_ctzll(act);
            const int b0 = __builtin_amdgcn_readlane(bin, first);
            if (__ballot(part && bin == b0) == act) {
              if (lane == first) atomicAdd(&hist[w][b0], (uint32_t)__popcll(act));
            } else if (part) {
              atomicAdd(&hist[w][bin], 1u);
            }
          }
        }
      }
      __syncthreads();
      if (tid < 256) {
        uint32_t c = 0;
#pragma unroll
        for (int ww = 0; ww < kSelWaves; ++ww) c += hist[ww][tid];
        hist[0][tid] = c;  // (thread tid alone reads and writes column tid)
      }
      __syncthreads();
      if (w == 0) {
        // suffix scan of the 256 bins, 4 per lane: sfx[j] = keys in the bins >= 4 lane + j.  The k-th key of the
        // prefix (rank need = k - above) is in the highest bin whose suffix count reaches need; no such bin
        // (fewer keys than k, first pass only): bin 0, every key is taken.
        uint32_t c[4], sfx[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = hist[0][4 * lane + j];
        uint32_t run = c[0] + c[1] + c[2] + c[3];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t v = __shfl_down(run, d);
          if (lane + d < 64) run += v;
        }
        sfx[3] = run - (c[0] + c[1] + c[2]);
        sfx[2] = sfx[3] + c[2];
        sfx[1] = sfx[2] + c[1];
        sfx[0] = sfx[1] + c[0];
        const uint32_t need = (uint32_t)k - above;
        int reach = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) reach += (int)__popcll(__ballot(sfx[j] >= need));
        const int b = max(reach - 1, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (4 * lane + j == b) {
            s_bin = (uint32_t)b;
            s_inbin = c[j];
            s_above = sfx[j] - c[j];
          }
      }
      __syncthreads();
      lo |= (uint64_t)s_bin << shift;
      pmask |= 0xffull << shift;
      above += s_above;
      if (above + s_inbin <= (uint32_t)N2) break;  // (uniform; distinct rows: one key per bin after the 8th pass)
    }
  }
  // gather: the keys above the prefix and in its bin are the non-zero keys >= lo, at most 2 * KB of them
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  for (int i0 = 0; i0 < nv; i0 += kSelThreads) {
    const int i = i0 + tid;
    u64x2 v = {0ull, 0ull};
    if (i < nv) v = kv[i];
    const uint64_t two[2] = {v.x, 2 * i + 1 < n ? v.y : 0ull};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint64_t key = two[h];
      const int slot = cand_claim(key != 0 && key >= lo, ~0ull, &s_cnt);
      if (slot >= 0 && slot < N2) buf[slot] = key;
    }
  }
  __syncthreads();
  for (int i = min(s_cnt, N2) + tid; i < N2; i += kSelThreads) buf[i] = 0;
  __syncthreads();
  cand_sort(buf, N2, 1u, N2);
  cand_write(buf, q, k, out_s, out_r);
}

// ---- the order of the re-ranked candidates -----------------------------------------------------------------------
// One workgroup per question: its n (score, row) pairs as keys into LDS, NS = n rounded up to 128 .. 1,024 sorted.
__global__ __launch_bounds__(kSelThreads) void deep_order_kernel(const float* __restrict__ s, const int64_t* __restrict__ r,
                                                                 int n, int NS, int k, float* __restrict__ out_s,
                                                                 int64_t* __restrict__ out_r) {
  __shared__ uint64_t buf[kDeepMaxK];
  const int64_t q = blockIdx.x;
  for (int i = threadIdx.x; i < NS; i += kSelThreads) {
    uint64_t key = 0;
    if (i < n) {
      const float sc = s[q * n + i];
      const int64_t row = r[q * n + i];
      if (row >= 0 && sc == sc) key = cand_key(sc, (int)row);  // a NaN score: a tombstoned row
    }
    buf[i] = key;
  }
  __syncthreads();
  cand_sort(buf, NS, 1u, NS);
  cand_write(buf, q, k, out_s, out_r);
}

}  // namespace

int launch_deep_select(const uint64_t* slab, int64_t qcap, const int* n_keys, int64_t nq, int k, float* out_s,
                       int64_t* out_r, hipStream_t st) {
  if (k < kDeepMinK || k > kDeepMaxK || nq < 1 || (qcap & 1) || ((uintptr_t)slab & 15)) return -1;
  hipLaunchKernelGGL(deep_select_kernel, dim3((unsigned)nq), dim3(kSelThreads), 0, st, slab, qcap, n_keys, deep_kb(k), k,
                     out_s, out_r);
  return 0;
}

int launch_deep_order(const float* s, const int64_t* r, int64_t nq, int n, int k, float* out_s, int64_t* out_r,
                      hipStream_t st) {
  if (n < 1 || n > kDeepMaxK || k < 1 || k > n || nq < 1) return -1;
  hipLaunchKernelGGL(deep_order_kernel, dim3((unsigned)nq), dim3(kSelThreads), 0, st, s, r, n, deep_kb(n), k, out_s,
                     out_r);
  return 0;
}

}  // namespace rfx
