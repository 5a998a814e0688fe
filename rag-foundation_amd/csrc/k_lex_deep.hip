// k_lex_deep.hip — the deep BM25 scan kernel and its launchers (see k_lex_deep.h; rules: DESIGN §4.14, §4.21).
#include "k_lex_deep.h"

#include "k_cand_keys.h"
#include "k_lex_score.h"

namespace rfx {
namespace {

constexpr int kLexWaves = kLexThreads / kWave;
static_assert(kLexWaves * 32 == kLexDeepRound, "a round is one 32-row tile per wave");

template <int NQT, bool LDS>
__global__ __launch_bounds__(kLexThreads) void lex_deep_scan_kernel(
    int V, const int64_t* __restrict__ indptr, const uint32_t* __restrict__ entries, const int32_t* __restrict__ len,
    int64_t rows, const float* __restrict__ W, int64_t nq, double k1, double b, double avgdl,
    const uint32_t* __restrict__ mask, int kb, int cap, uint64_t* __restrict__ slab, int* __restrict__ n_keys) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) uint8_t lex_deep_lds[];  // buffers [NQT][cap] u64, then the table
  __shared__ uint64_t s_tau[NQT];
  __shared__ int s_fill[NQT];
  __shared__ int s_cut[2];  // [round & 1]: a buffer passed the limit in that round
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int g = blockIdx.y;
  uint64_t* buf = (uint64_t*)lex_deep_lds;
  const float* Wg = W + (size_t)g * V * NQT;
  const float* wt = Wg;
  if constexpr (LDS) {
    float* wl = (float*)(lex_deep_lds + (size_t)NQT * cap * 8);
    for (int i = tid; i < V * NQT; i += kLexThreads) wl[i] = Wg[i];
    wt = wl;
  }
  if (tid < NQT) s_tau[tid] = 0, s_fill[tid] = 0;
  if (tid < 2) s_cut[tid] = 0;
  __syncthreads();
  const double k1p1 = k1 + 1.0;
  const double omb = 1.0 - b;
  const int64_t n_tiles = (rows + 31) >> 5;
  const int64_t n_waves = (int64_t)gridDim.x * kLexWaves;
  // A buffer that starts a round at or below `limit` holds the round's keys whatever they are.
  const int limit = cap - kLexDeepRound;
  int par = 0;
  // the trip count depends on the block alone: every wave of the workgroup meets after every round
  for (int64_t t0 = (int64_t)blockIdx.x * kLexWaves; t0 < n_tiles; t0 += n_waves, par ^= 1) {
    const int64_t t = t0 + w;
    uint32_t mword = 0u;  // wave-uniform; 0: no row of the tile is read
    if (t < n_tiles) mword = mask ? mask[t] : 0xffffffffu;
    if (mword != 0u) {
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
          const uint64_t key = cand_key((float)sum, (int)(r0 + rj[u]));
#pragma unroll
          for (int q = 0; q < NQT; ++q)
            if (lane == lex_owner_lane<NQT>(q) && sum > 0.0 && key > s_tau[q]) {
              const int slot = atomicAdd(&s_fill[q], 1);
              if (slot < cap) buf[(size_t)q * cap + slot] = key;  // (always: see `limit`)
              if (slot >= limit) s_cut[par] = 1;                  // the fill is now slot + 1 > limit
            }
        }
      }
    }
    __syncthreads();
    if (s_cut[par]) {    // workgroup-uniform: this round's flag is written again two rounds on at the earliest
      __syncthreads();   // every thread has read it
      if (tid == 0) s_cut[par] = 0;
      uint32_t need = 0;
#pragma unroll
      for (int q = 0; q < NQT; ++q) need |= (s_fill[q] > limit ? 1u : 0u) << q;
      cand_cut(buf, cap, kb, need, s_fill, s_tau);
    }
  }
  // ---- the block's kb best of every question -> its run of the slab ------------------------------------------
  const int nlive = (int)max((int64_t)0, min((int64_t)NQT, nq - (int64_t)g * NQT));  // the group's questions (uniform)
  cand_cut(buf, cap, kb, (1u << nlive) - 1u, s_fill, s_tau);
  for (int q = 0; q < nlive; ++q) {
    const int64_t gq = (int64_t)g * NQT + q;
    uint64_t* run = slab + ((size_t)gq * gridDim.x + blockIdx.x) * kb;
    for (int i = tid; i < kb; i += kLexThreads) run[i] = buf[(size_t)q * cap + i];
    if (blockIdx.x == 0 && tid == 0) n_keys[gq] = (int)gridDim.x * kb;
  }
}

__global__ void lex_deep_none_kernel(float* __restrict__ scores, int64_t* __restrict__ rows, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) scores[i] = -__builtin_inff(), rows[i] = -1;
}

template <int NQT, bool LDS>
int launch_deep_scan_t(const LexDeepPlan& p, int V, const int64_t* indptr, const uint32_t* entries, const int32_t* len,
                       int64_t rows, const float* W, int64_t nq, double k1, double b, double avgdl, const uint32_t* mask,
                       uint64_t* slab, int* n_keys, hipStream_t st) {
  auto kern = lex_deep_scan_kernel<NQT, LDS>;
  const size_t lds = (size_t)NQT * p.cap * 8 + (LDS ? (size_t)V * NQT * 4 : 0);
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return -1;
  hipLaunchKernelGGL(kern, dim3((unsigned)p.blocks, (unsigned)p.groups), dim3(kLexThreads), lds, st, V, indptr, entries,
                     len, rows, W, nq, k1, b, avgdl, mask, p.kb, p.cap, slab, n_keys);
  return 0;
}

}  // namespace

LexDeepPlan lex_deep_plan(int64_t rows, int V, int64_t nq, int k, int block_cap) {
  LexDeepPlan p{};
  p.nqt = nq <= 1 ? 1 : kLexDeepGroup;
  p.groups = (int)std::max<int64_t>(1, (nq + p.nqt - 1) / p.nqt);
  p.kb = deep_kb(k);
  p.cap = std::max(1024, 2 * p.kb);
  // a wave's share is whole 32-row tiles; few blocks per question when there are many questions, so that the
  // slab (nq * blocks * kb keys) stays bounded: 16 MB at 1,024 questions and kb 1,024
  const int64_t tiles = (std::max<int64_t>(rows, 1) + 31) / 32;
  const int64_t most = std::min<int64_t>(kLexBlocks, std::max<int64_t>(1, (tiles + 15) / 16));
  p.blocks = (int)std::min<int64_t>(most, std::max<int64_t>(1, kLexDeepTargetWgs / p.groups));
  if (block_cap > 0) p.blocks = std::min(p.blocks, block_cap);
  p.lds = V <= kLexLdsV;
  return p;
}

int launch_lex_deep_scan(const LexDeepPlan& p, int V, const int64_t* indptr, const uint32_t* entries, const int32_t* len,
                         int64_t rows, const float* W, int64_t nq, double k1, double b, double avgdl,
                         const uint32_t* mask, uint64_t* slab, int* n_keys, hipStream_t st) {
  if (rows < 1 || rows >= 0x7fffffffll || V < 1 || V > kLexMaxV || nq < 1 || nq > kLexMaxNq) return -1;
  if (!indptr || !len || !W || !slab || !n_keys) return -1;
  if (p.kb < 128 || p.kb > kDeepMaxK || p.cap < 2 * kLexDeepRound || (p.cap & (p.cap - 1)) ||
      p.kb > p.cap - kLexDeepRound || p.blocks < 1 || (p.nqt != 1 && p.nqt != kLexDeepGroup) ||
      (int64_t)p.groups * p.nqt < nq)
    return -1;
#define RFX_LEXD_ARGS p, V, indptr, entries, len, rows, W, nq, k1, b, avgdl, mask, slab, n_keys, st
  if (p.nqt == 1) return p.lds ? launch_deep_scan_t<1, true>(RFX_LEXD_ARGS) : launch_deep_scan_t<1, false>(RFX_LEXD_ARGS);
  return p.lds ? launch_deep_scan_t<kLexDeepGroup, true>(RFX_LEXD_ARGS)
               : launch_deep_scan_t<kLexDeepGroup, false>(RFX_LEXD_ARGS);
#undef RFX_LEXD_ARGS
}

void launch_lex_deep_none(float* scores, int64_t* rows, int64_t n, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(lex_deep_none_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, scores, rows, n);
}

}  // namespace rfx
