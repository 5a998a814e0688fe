// k_deep_f32.hip — the deep scan for f32 stores (k_deep_f32.h): resident f32 question fragments, rows streamed
// as a ring over (tile, 32-column block), v_mfma_f32_16x16x4_f32.  gfx950 only.
#include "k_deep_f32.h"

#include "k_deep.h"
#include "k_deep_buf.h"
#include "k_mfma_common.h"

namespace rfx {
namespace {

using mfc::v4f32x4;

constexpr int kBlkCols = 32;      // columns of a ring step: one 128-B line per row
constexpr int kBlkVecs = 8;       // 16-B vectors of a block (a lane loads vectors 2 g and 2 g + 1)
constexpr int R = kDeepF32Ring;

// A tile's scores against the lane's threshold: as the epilogue of k_deep.hip's tile.  The lane holds rows
// r0 + 4 g + i of question n; `bits` are the tile's live bits (wave-uniform).
__device__ __forceinline__ void deep_f32_select(const v4f32x4& acc, uint32_t bits, float thr, int r0, int n, int g,
                                                const DeepBuf& B) {
  const uint32_t nb = bits >> (4 * g);
  bool p[4];
  bool any = false;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    p[i] = acc[i] > thr && ((nb >> i) & 1u);  // NaN (a tombstoned row) never passes
    any |= p[i];
  }
  if (!__ballot(any)) return;  // no passer: no LDS traffic
  const int N = 2 * B.KB;
  const uint64_t mine = 0x0001000100010001ull << n;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int slot = cand_claim(p[i], mine, &B.cnt[n]);
    if (slot >= 0 && slot < N) B.buf[(size_t)n * N + slot] = cand_key(acc[i], r0 + 4 * g + i);
  }
}

// NBLK: the row's 32-column blocks, D / 32.  One instantiation per block count, not per 256 columns with a run-time
// count: behind a run-time test of the block the compiler can no longer count the loads in flight, and every wait
// of the ring becomes vmcnt(0).  A tile takes NSTEP steps, NBLK rounded up to the ring depth, so that a step's ring
// slot is static; the steps past NBLK neither load nor multiply (the ring is shallower there).
template <int NBLK>
__global__ __launch_bounds__(kDeepThreads) void deep_scan_f32_kernel(const uint8_t* __restrict__ X, int nrows, int D,
                                                                     const uint8_t* __restrict__ Q, int nq,
                                                                     const uint32_t* __restrict__ mask, DeepPlan P,
                                                                     uint64_t* __restrict__ ws) {
  constexpr int NSTEP = (NBLK + R - 1) / R * R;
  extern __shared__ __attribute__((aligned(16))) uint64_t deep_lds[];
  const int QG = P.q_per_wg, KB = P.kb, N = 2 * KB;
  const DeepBuf B(deep_lds, QG, KB);
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q0 = blockIdx.y * QG;
  const bool qlive = n < QG && q0 + n < nq;
  const int r_lo = (int)min((int64_t)blockIdx.x * P.rows_per_range, (int64_t)nrows);
  const int r_hi = (int)blockIdx.x == P.ranges - 1 ? nrows : r_lo + P.rows_per_range;
  if (tid < kDeepQSlots) {
    B.cnt[tid] = 0;
    B.tau[tid] = 0;
  }
  __syncthreads();

  // resident questions: block b's registers 8 b .. 8 b + 7 = columns 32 b + 8 g .. + 7 of question n
  v4f32x4 bq[2 * NBLK];
  {
    const v4f32x4* src = (const v4f32x4*)(Q + (int64_t)(qlive ? q0 + n : 0) * D * 4 + g * 32);
#pragma unroll
    for (int b = 0; b < NBLK; ++b) {
      bq[2 * b] = bq[2 * b + 1] = v4f32x4{0.f, 0.f, 0.f, 0.f};
      if (qlive) {
        bq[2 * b] = src[b * kBlkVecs];
        bq[2 * b + 1] = src[b * kBlkVecs + 1];
      }
    }
  }
  // a lane of no question (past the group, past nq) never passes
  float thr = qlive ? -__builtin_inff() : __builtin_inff();

  const int T = (r_hi - r_lo + kDeepRound - 1) / kDeepRound;  // rounds: one tile per wave each
  const int lim = N - P.check_rounds * kDeepRound;
  auto tile_row = [&](int t) { return (int64_t)r_lo + ((int64_t)t * 4 + wave) * 16; };
  // the lane's row of tile t at its bytes of block 0; a row past the range reads the range's last row (its live
  // bit is clear), so the ring's loads past the last tile stay inside the store
  auto tile_src = [&](int t) {
    const int64_t row = min(tile_row(t) + n, (int64_t)r_hi - 1);
    return (const v4f32x4*)(X + row * D * 4 + g * 32);
  };
  // bit i set = row r0 + i is inside the range and selected by the mask (wave-uniform: a scalar load)
  auto tile_bits = [&](int t) -> uint32_t {
    const int64_t r0 = tile_row(t);
    if (r0 >= r_hi) return 0u;
    uint32_t w = mask ? mask[r0 >> 5] >> (r0 & 31) : 0xffffu;
    w &= 0xffffu;
    if (r_hi - r0 < 16) w &= (1u << (int)(r_hi - r0)) - 1u;
    return w;
  };

  if (T > 0) {
    v4f32x4 ring[R][2];
    const v4f32x4* cur = tile_src(0);
    uint32_t bits = tile_bits(0);
#pragma unroll
    for (int s = 0; s < R; ++s) {
      if (s < NBLK) {
        ring[s][0] = __builtin_nontemporal_load(cur + s * kBlkVecs);
        ring[s][1] = __builtin_nontemporal_load(cur + s * kBlkVecs + 1);
      }
      __builtin_amdgcn_sched_barrier(0);  // oldest first, as the loop leaves the ring: its waits are counted
    }
    for (int t = 0; t < T; ++t) {
      // the next tile's address and live bits come before this tile's loads: nothing younger than a ring load
      // is ever waited for
      const v4f32x4* nxt = tile_src(t + 1);
      const uint32_t bits_n = tile_bits(t + 1);
      v4f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int b = 0; b < NSTEP; ++b) {
        if (b < NBLK) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {  // two accumulator chains, summed at the tile's end
            const float a = ring[b % R][j >> 2][j & 3], q = bq[2 * b + (j >> 2)][j & 3];
            if (j & 1)
              acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, q, acc1, 0, 0, 0);
            else
              acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, q, acc0, 0, 0, 0);
          }
        }
        // the slot is free: step b + R of this tile, or step b + R - NSTEP of the next one
        const int bn = (b + R) % NSTEP;
        if (bn < NBLK) {
          const v4f32x4* src = (b + R < NSTEP ? cur : nxt) + bn * kBlkVecs;
          ring[b % R][0] = __builtin_nontemporal_load(src);
          ring[b % R][1] = __builtin_nontemporal_load(src + 1);
        }
        // nothing crosses a step: left alone, the scheduler hoists a tile's loads to its top, which keeps the
        // whole tile live and ends in one load in flight at a time
        __builtin_amdgcn_sched_barrier(0);
      }
      deep_f32_select(acc0 + acc1, bits, thr, (int)tile_row(t), n, g, B);
      if ((t + 1) % P.check_rounds == 0 && deep_compact(B, QG, lim) && qlive) {
        const uint64_t tk = B.tau[n];
        thr = tk ? cand_key_score(tk) : -__builtin_inff();
      }
      cur = nxt;
      bits = bits_n;
    }
  }
  deep_compact(B, QG, -1);
  for (int i = tid; i < QG * KB; i += kDeepThreads) {
    const int q = i / KB, j = i - q * KB;
    if (q0 + q < nq) ws[((size_t)(q0 + q) * P.ranges + blockIdx.x) * KB + j] = B.buf[(size_t)q * N + j];
  }
}

template <int NBLK>
int launch_scan(const DeepPlan& p, const void* X, int nrows, int D, const void* Q, int nq, const uint32_t* mask, uint64_t* ws,
                hipStream_t st) {
  auto kern = deep_scan_f32_kernel<NBLK>;
  const size_t lds = deep_lds_bytes(p.q_per_wg, p.kb);
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return -1;
  hipLaunchKernelGGL(kern, dim3((unsigned)p.ranges, (unsigned)p.q_groups), dim3(kDeepThreads), lds, st, (const uint8_t*)X,
                     nrows, D, (const uint8_t*)Q, nq, mask, p, ws);
  return 0;
}

}  // namespace

int launch_deep_search_f32(const DeepPlan& p, const void* X, int64_t nrows, int D, const void* Q, int64_t nq, int k,
                           const uint32_t* mask, uint64_t* ws, float* out_s, int64_t* out_r, hipStream_t st) {
  if (!deep_launch_ok(p, nrows, D, nq, k)) return -1;
  int rc = -1;
  switch (D / kBlkCols) {
#define RFX_DEEP_F32_CASE(NB) \
  case NB: rc = launch_scan<NB>(p, X, (int)nrows, D, Q, (int)nq, mask, ws, st); break;
    RFX_DEEP_F32_CASE(2) RFX_DEEP_F32_CASE(4) RFX_DEEP_F32_CASE(6) RFX_DEEP_F32_CASE(8)
    RFX_DEEP_F32_CASE(10) RFX_DEEP_F32_CASE(12) RFX_DEEP_F32_CASE(14) RFX_DEEP_F32_CASE(16)
    RFX_DEEP_F32_CASE(18) RFX_DEEP_F32_CASE(20) RFX_DEEP_F32_CASE(22) RFX_DEEP_F32_CASE(24)
    RFX_DEEP_F32_CASE(26) RFX_DEEP_F32_CASE(28) RFX_DEEP_F32_CASE(30) RFX_DEEP_F32_CASE(32)
#undef RFX_DEEP_F32_CASE
  }
  if (rc) return rc;
  launch_deep_merge(p, X, nrows, D, RFX_F32, Q, nq, k, ws, out_s, out_r, st);
  return 0;
}

}  // namespace rfx
