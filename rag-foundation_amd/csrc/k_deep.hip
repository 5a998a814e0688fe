// k_deep.hip — the deep search kernels (k_deep.h): scan with threshold + LDS buffer + periodic sort, and the
// per-question merge with the f64 re-score.  Keys, slot claim, sort and cut: k_cand_keys.h; the buffers and the
// meeting, shared with the f32 scan: k_deep_buf.h.  gfx950 only.
#include "k_deep.h"

#include "k_deep_buf.h"
#include "k_mfma_common.h"
#include "k_scan_valu.h"  // rescore_dot: the score rule's f64 dot

namespace rfx {
namespace {

using mfc::v4f32x4;

// ---- scan ---------------------------------------------------------------------------------------------------
// A fragments of the 16-row tile at r0 (NDS * 64 columns at most, nds * 64 in use) and the tile's live bits:
// bit i set = row r0 + i is inside the range and selected by the mask.  A tile past the range loads nothing.
template <int NDS>
__device__ __forceinline__ void deep_load_tile(uint4 (&a)[2 * NDS], uint32_t& bits, const uint8_t* __restrict__ X, int D,
                                               int nds, int r0, int r_hi, const uint32_t* __restrict__ mask, int n,
                                               int g) {
  bits = 0;
  if (r0 >= r_hi) return;
  const int left = r_hi - r0;
  uint32_t w = mask ? mask[r0 >> 5] >> (r0 & 31) : 0xffffu;
  w &= 0xffffu;
  if (left < 16) w &= (1u << left) - 1u;
  bits = w;
  const int row = min(r0 + n, r_hi - 1);  // a row past the range: any row of it (its bit is clear)
  const mfc::v4i32* src = (const mfc::v4i32*)(X + (int64_t)row * D * 2 + g * 32);  // read once: non-temporal
#pragma unroll
  for (int ds = 0; ds < NDS; ++ds)
    if (ds < nds) {
      a[2 * ds] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(src + ds * 8));
      a[2 * ds + 1] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(src + ds * 8 + 1));
    }
}

// One tile against the resident questions: 2 * nds MFMAs, one compare per accumulator register, one ballot.
template <int DT, int NDS>
__device__ __forceinline__ void deep_use_tile(const uint4 (&a)[2 * NDS], uint32_t bits, const uint4 (&bq)[2 * NDS], int nds,
                                              float thr, int r0, int n, int g, const DeepBuf& B) {
  if (!bits) return;  // (wave-uniform)
  v4f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ds = 0; ds < NDS; ++ds)
    if (ds < nds) {
      acc0 = mfc::mfma16<DT>(a[2 * ds], bq[2 * ds], acc0);
      acc1 = mfc::mfma16<DT>(a[2 * ds + 1], bq[2 * ds + 1], acc1);
    }
  const v4f32x4 acc = acc0 + acc1;
  const uint32_t nb = bits >> (4 * g);
  bool p[4];
  bool any = false;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    p[i] = acc[i] > thr && ((nb >> i) & 1u);  // NaN (a tombstoned row) never passes
    any |= p[i];
  }
  if (!__ballot(any)) return;
  const int N = 2 * B.KB;
  const uint64_t mine = 0x0001000100010001ull << n;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int slot = cand_claim(p[i], mine, &B.cnt[n]);
    if (slot >= 0 && slot < N) B.buf[(size_t)n * N + slot] = cand_key(acc[i], r0 + 4 * g + i);
  }
}

template <int DT, int NDS>
__global__ __launch_bounds__(kDeepThreads) void deep_scan_kernel(const uint8_t* __restrict__ X, int nrows, int D,
                                                                 const uint8_t* __restrict__ Q, int nq,
                                                                 const uint32_t* __restrict__ mask, DeepPlan P,
                                                                 uint64_t* __restrict__ ws,
                                                                 const int* __restrict__ nq_dev) {
  extern __shared__ __attribute__((aligned(16))) uint64_t deep_lds[];
  const int QG = P.q_per_wg, KB = P.kb, N = 2 * KB;
  if (nq_dev) {  // a question count that is known on the device only: groups past it exit at once (uniform)
    nq = min(nq, *nq_dev);
    if ((int)blockIdx.y * QG >= nq) return;
  }
  const DeepBuf B(deep_lds, QG, KB);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.y * QG;
  const bool qlive = n < QG && q0 + n < nq;
  const int r_lo = (int)min((int64_t)blockIdx.x * P.rows_per_range, (int64_t)nrows);
  const int r_hi = (int)blockIdx.x == P.ranges - 1 ? nrows : r_lo + P.rows_per_range;
  const int nds = D >> 6;
  if (tid < kDeepQSlots) {
    B.cnt[tid] = 0;
    B.tau[tid] = 0;
  }
  __syncthreads();

  uint4 bq[2 * NDS];
  {
    const uint4* src = (const uint4*)(Q + (int64_t)(qlive ? q0 + n : 0) * D * 2 + g * 32);
#pragma unroll
    for (int ds = 0; ds < NDS; ++ds) {
      bq[2 * ds] = bq[2 * ds + 1] = make_uint4(0, 0, 0, 0);
      if (ds < nds && qlive) {
        bq[2 * ds] = src[ds * 8];
        bq[2 * ds + 1] = src[ds * 8 + 1];
      }
    }
  }
  // a lane of no question (past the group, past nq) never passes
  float thr = qlive ? -__builtin_inff() : __builtin_inff();

  const int T = (r_hi - r_lo + kDeepRound - 1) / kDeepRound;  // rounds: one tile per wave each
  const int lim = N - P.check_rounds * kDeepRound;
  uint4 a0[2 * NDS], a1[2 * NDS];
  uint32_t bits0 = 0, bits1 = 0;
  auto tile_row = [&](int t) { return r_lo + (t * 4 + wave) * 16; };
  if (T > 0) deep_load_tile<NDS>(a0, bits0, X, D, nds, tile_row(0), r_hi, mask, n, g);
  for (int t = 0; t < T; t += 2) {
    if (t + 1 < T) deep_load_tile<NDS>(a1, bits1, X, D, nds, tile_row(t + 1), r_hi, mask, n, g);
    deep_use_tile<DT, NDS>(a0, bits0, bq, nds, thr, tile_row(t), n, g, B);
    if (t + 1 < T) {
      if (t + 2 < T) deep_load_tile<NDS>(a0, bits0, X, D, nds, tile_row(t + 2), r_hi, mask, n, g);
      deep_use_tile<DT, NDS>(a1, bits1, bq, nds, thr, tile_row(t + 1), n, g, B);
    }
    // (check_rounds is even: a meeting falls after the second tile of a pair)
    if ((t + 2) % P.check_rounds == 0 && deep_compact(B, QG, lim) && qlive) {
      const uint64_t tk = B.tau[n];
      thr = tk ? cand_key_score(tk) : -__builtin_inff();
    }
  }
  deep_compact(B, QG, -1);
  for (int i = tid; i < QG * KB; i += kDeepThreads) {
    const int q = i / KB, j = i - q * KB;
    if (q0 + q < nq) ws[((size_t)(q0 + q) * P.ranges + blockIdx.x) * KB + j] = B.buf[(size_t)q * N + j];
  }
}

// ---- merge --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDeepThreads) void deep_merge_kernel(const uint64_t* __restrict__ ws, int ranges, int KB, int k,
                                                                  const void* __restrict__ X, int nrows, int D, int dtype,
                                                                  const void* __restrict__ Q, float* __restrict__ out_s,
                                                                  int64_t* __restrict__ out_r,
                                                                  const int* __restrict__ nq_dev) {
  extern __shared__ __attribute__((aligned(16))) uint64_t deep_lds[];
  if (nq_dev && (int)blockIdx.x >= *nq_dev) return;  // (uniform)
  const DeepBuf B(deep_lds, 1, KB);
  const int tid = threadIdx.x, N = 2 * KB;
  const int64_t q = blockIdx.x;
  if (tid < kDeepQSlots) {
    B.cnt[tid] = 0;
    B.tau[tid] = 0;
  }
  __syncthreads();
  const int total = ranges * KB, R = min(kDeepThreads, KB), lim = N - R;
  const uint64_t* src = ws + (size_t)q * total;
  for (int base = 0; base < total; base += R) {
    const int i = base + tid;
    const uint64_t key = tid < R && i < total ? src[i] : 0;
    const bool pass = key > B.tau[0];  // the full key: equal scores of different ranges go to the lower row
    const int slot = cand_claim(pass, ~0ull, &B.cnt[0]);
    if (slot >= 0 && slot < N) B.buf[slot] = key;
    deep_compact(B, 1, lim);
  }
  deep_compact(B, 1, -1);  // buf[0 .. KB): the best, in order; empty places (key 0) last

  // the score rule of every search: fl32 of the f64 dot of the stored values (8 lanes per entry), then the
  // order again under the new scores
  const int gl = tid & 7;
  for (int e0 = 0; e0 < KB; e0 += kDeepThreads / 8) {
    const int e = e0 + (tid >> 3);
    const uint64_t key = e < k ? B.buf[e] : 0;
    int row = key ? cand_key_row(key) : -1;
    if (row >= nrows) row = -1;
    const double acc = rescore_dot(X, row, Q, q, D, dtype, gl, row >= 0);
    if (gl == 0) B.buf[KB + e] = row >= 0 ? cand_key((float)acc, row) : 0;
  }
  __syncthreads();
  cand_sort(B.buf + KB, KB, 1u, KB);
  cand_write(B.buf + KB, q, k, out_s, out_r);
}

template <int DT, int NDS>
int launch_scan(const DeepPlan& p, const void* X, int nrows, int D, const void* Q, int nq, const uint32_t* mask, uint64_t* ws,
                const int* nq_dev, hipStream_t st) {
  auto kern = deep_scan_kernel<DT, NDS>;
  const size_t lds = deep_lds_bytes(p.q_per_wg, p.kb);
  if (lds > (size_t)kDeepLdsBudget) return -1;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return -1;
  hipLaunchKernelGGL(kern, dim3((unsigned)p.ranges, (unsigned)p.q_groups), dim3(kDeepThreads), lds, st, (const uint8_t*)X,
                     nrows, D, (const uint8_t*)Q, nq, mask, p, ws, nq_dev);
  return 0;
}

template <int DT>
int launch_scan_dt(const DeepPlan& p, const void* X, int nrows, int D, const void* Q, int nq, const uint32_t* mask,
                   uint64_t* ws, const int* nq_dev, hipStream_t st) {
  switch ((D / 64 + 3) / 4) {
    case 1: return launch_scan<DT, 4>(p, X, nrows, D, Q, nq, mask, ws, nq_dev, st);
    case 2: return launch_scan<DT, 8>(p, X, nrows, D, Q, nq, mask, ws, nq_dev, st);
    case 3: return launch_scan<DT, 12>(p, X, nrows, D, Q, nq, mask, ws, nq_dev, st);
    case 4: return launch_scan<DT, 16>(p, X, nrows, D, Q, nq, mask, ws, nq_dev, st);
  }
  return -1;
}

}  // namespace

void launch_deep_merge(const DeepPlan& p, const void* X, int64_t nrows, int D, int dtype, const void* Q, int64_t nq, int k,
                       const uint64_t* ws, float* out_s, int64_t* out_r, hipStream_t st, const int* nq_dev) {
  hipLaunchKernelGGL(deep_merge_kernel, dim3((unsigned)nq), dim3(kDeepThreads), deep_lds_bytes(1, p.kb), st, ws, p.ranges, p.kb,
                     k, X, (int)nrows, D, dtype, Q, out_s, out_r, nq_dev);
}

int launch_deep_search(const DeepPlan& p, const void* X, int64_t nrows, int D, int dtype, const void* Q, int64_t nq, int k,
                       const uint32_t* mask, uint64_t* ws, float* out_s, int64_t* out_r, hipStream_t st, const int* nq_dev) {
  if ((dtype != RFX_BF16 && dtype != RFX_F16) || !deep_launch_ok(p, nrows, D, nq, k)) return -1;
  const int rc = dtype == RFX_BF16 ? launch_scan_dt<RFX_BF16>(p, X, (int)nrows, D, Q, (int)nq, mask, ws, nq_dev, st)
                                   : launch_scan_dt<RFX_F16>(p, X, (int)nrows, D, Q, (int)nq, mask, ws, nq_dev, st);
  if (rc) return rc;
  launch_deep_merge(p, X, nrows, D, dtype, Q, nq, k, ws, out_s, out_r, st, nq_dev);
  return 0;
}

}  // namespace rfx
