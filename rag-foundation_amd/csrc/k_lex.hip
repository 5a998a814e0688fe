// k_lex.hip — the BM25 lexical scan kernels and their launchers (see k_lex.h; rules: DESIGN §4.14).
#include "k_lex.h"

#include "../../include/rfx.h"
#include "rfx_device.h"

namespace rfx {
namespace {

constexpr int kLexWaves = kLexThreads / kWave;

// ---- weight tables: W[g][bucket][q % NQT] = w, everything else 0 --------------------------------------
__global__ __launch_bounds__(1024) void lex_weights_kernel(int V, int nqt, const int32_t* __restrict__ q_off,
                                                           const LexQueryEntry* __restrict__ q_ent, int64_t nq,
                                                           float* __restrict__ W) {
  const int g = blockIdx.x;
  float* Wg = W + (size_t)g * V * nqt;
  for (int i = threadIdx.x; i < V * nqt; i += blockDim.x) Wg[i] = 0.0f;
  __syncthreads();  // (the block's own zeros are ordered before its own entries)
  for (int ql = 0; ql < nqt; ++ql) {
    const int64_t q = (int64_t)g * nqt + ql;
    if (q >= nq) break;
    // a question's buckets are distinct (lex_query_weights): no two threads write one word
    for (int e = q_off[q] + threadIdx.x; e < q_off[q + 1]; e += blockDim.x)
      if ((int)q_ent[e].bucket < V) Wg[(size_t)q_ent[e].bucket * nqt + ql] = q_ent[e].w;
  }
}

// One entry's contribution to the questions of the group: x = (tf * (k1 + 1)) / (tf + B_r), an IEEE f64
// division taken once per entry (it does not depend on the question), then acc_q += w_q * x with the product
// and the sum rounded on their own.
template <int NQT>
__device__ __forceinline__ void lex_accumulate(uint32_t e, double B, double k1p1, const float* __restrict__ wt,
                                               double (&acc)[NQT]) {
#pragma clang fp contract(off)
  const uint32_t tf = e >> 16;
  if (tf == 0u) return;  // no entry in this lane (a stored tf is >= 1)
  const float* wp = wt + (size_t)(e & 0xffffu) * NQT;
  float w[NQT];
  if constexpr (NQT == 8) {
    const float4 a = ((const float4*)wp)[0], b4 = ((const float4*)wp)[1];
    w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b4.x, w[5] = b4.y, w[6] = b4.z, w[7] = b4.w;
  } else {
#pragma unroll
    for (int q = 0; q < NQT; ++q) w[q] = wp[q];
  }
  bool any = false;
#pragma unroll
  for (int q = 0; q < NQT; ++q) any |= w[q] != 0.0f;
  if (!any) return;
  const double tfd = (double)tf;
  const double num = tfd * k1p1;
  const double den = tfd + B;
  const double x = num / den;
#pragma unroll
  for (int q = 0; q < NQT; ++q) {
    const double t = (double)w[q] * x;
    acc[q] = acc[q] + t;
  }
}

// The xor butterfly (32, 16, 8, 4, 2, 1) over NQT sums at once: at each of the first log2(NQT) steps a lane
// keeps half of its sums and hands the other half to its partner, so question q's sum pairs the same lanes in
// the same order as a butterfly over that sum alone (f64 addition commutes: the value is the lone butterfly's,
// whatever NQT).  Afterwards acc[0] of lane l is the sum of question lex_owner_q(l).
template <int NQT>
__device__ __forceinline__ double lex_reduce(double (&acc)[NQT], int lane) {
  int off = 32;
#pragma unroll
  for (int n = NQT; n > 1; n >>= 1) {
    const int half = n >> 1;
    const bool hi = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const double keep = hi ? acc[i + half] : acc[i];
      const double send = hi ? acc[i] : acc[i + half];
      acc[i] = keep + __shfl_xor(send, off);
    }
    off >>= 1;
  }
  for (; off; off >>= 1) acc[0] = acc[0] + __shfl_xor(acc[0], off);
  return acc[0];
}
// the first lane that holds question q's sum after lex_reduce
template <int NQT>
__device__ __forceinline__ int lex_owner_lane(int q) {
  int l = 0, off = 32;
  for (int n = NQT; n > 1; n >>= 1) {
    if (q & (n >> 1)) l |= off;
    off >>= 1;
  }
  return l;
}

__device__ __forceinline__ long long readlane_i64(long long v, int l) {
  return (long long)(((uint64_t)(uint32_t)readlane_i((int)(v >> 32), l) << 32) | (uint32_t)readlane_i((int)v, l));
}

// grid (blocks, groups).  A wave takes 32-row tiles (one row-mask word each), gw, gw + waves, ...; within a tile
// it takes the live, allowed, non-empty rows four at a time (four entry loads in flight), its lanes striding a
// row's entries: lane and trip of an entry depend on the row alone.
template <int K, int NQT, bool LDS>
__global__ __launch_bounds__(kLexThreads) void lex_scan_kernel(int V, const int64_t* __restrict__ indptr,
                                                               const uint32_t* __restrict__ entries,
                                                               const int32_t* __restrict__ len, int64_t rows,
                                                               const float* __restrict__ W, int64_t nq, double k1,
                                                               double b, double avgdl,
                                                               const uint32_t* __restrict__ mask,
                                                               float* __restrict__ cs, int* __restrict__ cr) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) uint8_t lex_lds[];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int g = blockIdx.y;
  const float* Wg = W + (size_t)g * V * NQT;
  const float* wt = Wg;
  if constexpr (LDS) {
    float* wl = (float*)lex_lds;
    for (int i = tid; i < V * NQT; i += kLexThreads) wl[i] = Wg[i];
    wt = wl;
    __syncthreads();
  }
  WaveList<K> L[NQT];
#pragma unroll
  for (int q = 0; q < NQT; ++q) L[q].init();
  const double k1p1 = k1 + 1.0;
  const double omb = 1.0 - b;
  const int64_t n_tiles = (rows + 31) >> 5;
  const int64_t n_waves = (int64_t)gridDim.x * kLexWaves;
  for (int64_t t = (int64_t)blockIdx.x * kLexWaves + w; t < n_tiles; t += n_waves) {
    const uint32_t mword = mask ? mask[t] : 0xffffffffu;  // wave-uniform
    if (mword == 0u) continue;                            // no row of the tile is read
    const int64_t r0 = t << 5;
    long long ip = 0;
    int ln = -1;
    if (lane <= 32) ip = indptr[min(r0 + lane, rows)];
    if (lane < 32 && r0 + lane < rows) ln = len[r0 + lane];
    uint32_t todo = (uint32_t)__ballot(lane < 32 && ln > 0) & mword;  // live, allowed, at least one entry
    while (todo) {
      int rj[4];
      long long s[4], e[4];
      uint32_t ent[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        rj[u] = -1;
        ent[u] = 0u;
        if (todo) {
          rj[u] = __builtin_ctz(todo);
          todo &= todo - 1;
          s[u] = readlane_i64(ip, rj[u]);
          e[u] = readlane_i64(ip, rj[u] + 1);
          if (s[u] + lane < e[u]) ent[u] = entries[s[u] + lane];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (rj[u] < 0) break;  // wave-uniform
        const double lr = (double)readlane_i(ln, rj[u]);
        const double rel = lr / avgdl;
        const double B = k1 * (omb + b * rel);
        double acc[NQT];
#pragma unroll
        for (int q = 0; q < NQT; ++q) acc[q] = 0.0;
        lex_accumulate<NQT>(ent[u], B, k1p1, wt, acc);
        for (long long i = s[u] + 64 + lane; i < e[u]; i += 64) lex_accumulate<NQT>(entries[i], B, k1p1, wt, acc);
        const double sum = lex_reduce<NQT>(acc, lane);
        const float sc = (float)sum;
        const int row = (int)(r0 + rj[u]);
#pragma unroll
        for (int q = 0; q < NQT; ++q) L[q].offer(sc, row, lane == lex_owner_lane<NQT>(q) && sum > 0.0);
      }
    }
  }
  // ---- the block's 16 wave lists of a question -> one list (wave q merges question q) -------------------
  __syncthreads();  // every wave is done with the weight table: its LDS is reused
  float* ms = (float*)lex_lds;                         // [waves][NQT][K]
  int* mr = (int*)(lex_lds + (size_t)kLexWaves * NQT * K * 4);
#pragma unroll
  for (int q = 0; q < NQT; ++q)
    if (lane < K) {
      ms[(w * NQT + q) * K + lane] = L[q].ls;
      mr[(w * NQT + q) * K + lane] = L[q].lr;
    }
  __syncthreads();
  if (w < NQT) {
    const int64_t q = (int64_t)g * NQT + w;
    if (q < nq) {  // wave-uniform
      WaveList<K> M;
      M.init();
      for (int sw = 0; sw < kLexWaves; ++sw) {
        float s1 = -__builtin_inff();
        int r1 = kEmptyRow;
        if (lane < K) {
          s1 = ms[(sw * NQT + w) * K + lane];
          r1 = mr[(sw * NQT + w) * K + lane];
        }
        M.offer(s1, r1, r1 != kEmptyRow);
      }
      if (lane < K) {
        const size_t o = ((size_t)q * gridDim.x + blockIdx.x) * K + lane;
        cs[o] = M.ls;
        cr[o] = M.lr;
      }
    }
  }
}

__global__ void lex_set_dead_kernel(int32_t* __restrict__ len, const int64_t* __restrict__ rows, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) len[rows[i]] = -1;
}

size_t lex_scan_lds(const LexPlan& p, int V) {
  const size_t table = p.lds ? (size_t)V * p.nqt * 4 : 0;
  const size_t merge = (size_t)kLexWaves * p.nqt * p.k_slot * 8;
  return std::max(table, merge);
}

template <int K, int NQT, bool LDS>
int launch_scan_t(const LexPlan& p, int V, const int64_t* indptr, const uint32_t* entries, const int32_t* len,
                  int64_t rows, const float* W, int64_t nq, double k1, double b, double avgdl, const uint32_t* mask,
                  float* cs, int* cr, hipStream_t st) {
  auto kern = lex_scan_kernel<K, NQT, LDS>;
  const size_t lds = lex_scan_lds(p, V);
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return -1;
  hipLaunchKernelGGL(kern, dim3((unsigned)p.blocks, (unsigned)p.groups), dim3(kLexThreads), lds, st, V, indptr, entries,
                     len, rows, W, nq, k1, b, avgdl, mask, cs, cr);
  return 0;
}

}  // namespace

LexPlan lex_plan(int64_t rows, int V, int64_t nq, int k) {
  LexPlan p{};
  p.nqt = nq <= 1 ? 1 : kLexGroup;
  p.groups = (int)((nq + p.nqt - 1) / p.nqt);
  // a wave's share is whole 32-row tiles: no more blocks than there are tiles for their waves
  const int64_t tiles = (rows + 31) / 32;
  p.blocks = (int)std::min<int64_t>(kLexBlocks, std::max<int64_t>(1, (tiles + kLexWaves - 1) / kLexWaves));
  p.k_slot = k <= 4 ? 4 : (k <= 16 ? 16 : 64);
  p.lds = V <= kLexLdsV;
  return p;
}

void launch_lex_weights(const LexPlan& p, int V, const int32_t* q_off, const LexQueryEntry* q_ent, int64_t nq, float* W,
                        hipStream_t st) {
  hipLaunchKernelGGL(lex_weights_kernel, dim3((unsigned)p.groups), dim3(1024), 0, st, V, p.nqt, q_off, q_ent, nq, W);
}

int launch_lex_scan(const LexPlan& p, int V, const int64_t* indptr, const uint32_t* entries, const int32_t* len,
                    int64_t rows, const float* W, int64_t nq, double k1, double b, double avgdl, const uint32_t* mask,
                    float* cs, int* cr, hipStream_t st) {
  if (rows < 1 || rows >= 0x7fffffffll || V < 1 || V > kLexMaxV || nq < 1 || nq > kLexMaxNq) return -1;
  if (!indptr || !len || !W || !cs || !cr) return -1;
#define RFX_LEX_ARGS p, V, indptr, entries, len, rows, W, nq, k1, b, avgdl, mask, cs, cr, st
#define RFX_LEX_K(KV)                                                                                  \
  if (p.k_slot == KV) {                                                                                \
    if (p.nqt == 1) return p.lds ? launch_scan_t<KV, 1, true>(RFX_LEX_ARGS) : launch_scan_t<KV, 1, false>(RFX_LEX_ARGS); \
    return p.lds ? launch_scan_t<KV, 8, true>(RFX_LEX_ARGS) : launch_scan_t<KV, 8, false>(RFX_LEX_ARGS); \
  }
  RFX_LEX_K(4)
  RFX_LEX_K(16)
  RFX_LEX_K(64)
#undef RFX_LEX_K
#undef RFX_LEX_ARGS
  return -1;
}

void launch_lex_set_dead(int32_t* len, const int64_t* rows_d, int64_t n, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(lex_set_dead_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, len, rows_d, n);
}

}  // namespace rfx
