// k_deep_sampled.hip — the sampled-threshold deep search (k_deep_sampled.h): the staged scan with its DENSE and
// THRESH epilogues, the small kernels between the passes, and the call that strings them together with the
// selection of k_deep_select.h and the fallback to k_deep.h.  Keys: k_cand_keys.h.  gfx950 only.
#include "k_deep_sampled.h"

#include "k_cand_keys.h"
#include "k_deep.h"
#include "k_deep_select.h"
#include "k_mfma_common.h"
#include "k_scan_valu.h"  // rescore_dot: the score rule's f64 dot

namespace rfx {
namespace {

using mfc::v4f32x4;

constexpr int kDsRowB = 512;                   // bytes of a row in a stage: 256 columns
constexpr int kDsStage = kDsRound * kDsRowB;   // 32 KiB: 64 rows x 256 columns
constexpr int kDsChunks = kDsStage / 16;       // 16-B chunks of a stage
constexpr int kDsTiles = kDsRound / 16;

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

struct DsScan {
  const uint8_t* X;
  const uint8_t* Q;
  const uint32_t* mask;  // optional row bitmap
  const float* tau;      // [nq], THRESH
  int* count;            // [nq], THRESH
  uint64_t* slab;        // [nq][slab_stride]
  int64_t slab_stride;
  int D, nq;
  int n_ord, stride;     // ordinals [0, n_ord): row o * stride
  int ord_per_range;     // a multiple of 64
  int narrow;            // 1: the 4 waves hold the same 16 questions and take one tile of a round each
  int thresh;            // 0: DENSE epilogue, 1: THRESH
  int cap;
};

// Two waves per SIMD (256 registers) wherever the resident questions leave room; the 4-wave form at dim > 512
// spills there (16..116 B of scratch), so it takes one wave per SIMD and 512 registers.  The 8-wave form cannot
// (8 waves on 4 SIMDs): it serves dim <= 768 only, where it fits (deep_sampled_plan).
template <int DT, int NDS, int WAVES>
__global__ __launch_bounds__(64 * WAVES, (WAVES == 4 && NDS >= 12) ? 1 : 2) void deep_sampled_scan_kernel(const DsScan a) {
  constexpr int NT = 64 * WAVES, LPT = kDsChunks / NT, NST = NDS / 4;  // loads per thread and stage; stages per round
  __shared__ __attribute__((aligned(1024))) uint8_t lds[2 * kDsStage];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, g = lane >> 4;
  const int D = a.D, nds = D >> 6;  // NDS = 4 * ceil(nds / 4): only the last stage can be short
  const int64_t o_first = (int64_t)blockIdx.x * a.ord_per_range;
  if (o_first >= a.n_ord) return;  // (uniform; not with the host's split)
  const int o_lo = (int)o_first, o_hi = (int)min((int64_t)a.n_ord, o_first + a.ord_per_range);
  const int q = (int)blockIdx.y * (a.narrow ? kDsNarrowQ : 16 * WAVES) + (a.narrow ? 0 : 16 * wave) + n;
  const bool qlive = q < a.nq;

  // resident questions: the B fragments, in the column permutation of the A fragments below (a lane's two
  // 16-B vectors of a 64-column block are bytes [32 g, 32 g + 32) of its 128 B; a dot product does not see it)
  uint4 bq[2 * NDS];
  {
    const uint4* src = (const uint4*)(a.Q + (int64_t)(qlive ? q : 0) * D * 2 + g * 32);
#pragma unroll
    for (int ds = 0; ds < NDS; ++ds) {
      bq[2 * ds] = bq[2 * ds + 1] = make_uint4(0, 0, 0, 0);
      if (ds < nds && qlive) {
        bq[2 * ds] = src[ds * 8];
        bq[2 * ds + 1] = src[ds * 8 + 1];
      }
    }
  }
  // a lane of no question never passes; -inf ("none") passes every eligible row
  const float thr = qlive ? (a.thresh ? a.tau[q] : -__builtin_inff()) : __builtin_inff();

  // staging: thread -> chunk c of rows r0 + (NT / 32) j of the round; rows past the range re-read its last row
  const int c = tid & 31, r0 = tid >> 5;
  auto load_stage = [&](uint4 (&pf)[LPT], int rnd, int cs) {
    if (c >= min(4, nds - 4 * cs) * 8) return;
    const int ob = o_lo + rnd * kDsRound;
#pragma unroll
    for (int j = 0; j < LPT; ++j) {
      const int64_t row = (int64_t)min(ob + r0 + (NT / 32) * j, o_hi - 1) * a.stride;
      const mfc::v4i32* src = (const mfc::v4i32*)(a.X + row * D * 2 + cs * kDsRowB + c * 16);
      pf[j] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(src));  // read once per question group
    }
  };
  auto store_stage = [&](const uint4 (&pf)[LPT], int slot, int cs) {
    if (c >= min(4, nds - 4 * cs) * 8) return;
#pragma unroll
    for (int j = 0; j < LPT; ++j) {
      const int r = r0 + (NT / 32) * j;
      *(uint4*)(lds + slot * kDsStage + r * kDsRowB + ((c ^ (r & 15)) << 4)) = pf[j];
    }
  };
  // lane l: is ordinal (round's first + l) inside the range and selected by the mask
  auto live_lane = [&](int rnd) -> bool {
    const int o = o_lo + rnd * kDsRound + lane;
    if (o >= o_hi) return false;
    if (!a.mask) return true;
    const int64_t row = (int64_t)o * a.stride;
    return (a.mask[row >> 5] >> (row & 31)) & 1u;
  };

  const int R = (o_hi - o_lo + kDsRound - 1) / kDsRound;
  uint4 pf[LPT];
  load_stage(pf, 0, 0);
  uint64_t bits = __ballot(live_lane(0)), bits_next = 0;
  store_stage(pf, 0, 0);
  __syncthreads();
  int slot = 0;
  for (int rnd = 0; rnd < R; ++rnd) {
    v4f32x4 acc[kDsTiles];
#pragma unroll
    for (int t = 0; t < kDsTiles; ++t) acc[t] = v4f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int cs = 0; cs < NST; ++cs) {
      // the next stage's loads go out before this stage's MFMAs and land in the other slot after them
      const bool wrap = cs + 1 == NST;
      const int nr = wrap ? rnd + 1 : rnd, ncs = wrap ? 0 : cs + 1;
      const bool more = nr < R;  // (uniform)
      bool live_next = false;
      if (more) load_stage(pf, nr, ncs);
      if (wrap && more) live_next = live_lane(nr);
      const uint8_t* img = lds + slot * kDsStage + n * kDsRowB;
#pragma unroll
      for (int t = 0; t < kDsTiles; ++t) {
        if (a.narrow && t != wave) continue;  // (wave-uniform)
#pragma unroll
        for (int dl = 0; dl < 4; ++dl) {
          const int ds = 4 * cs + dl;
          if (ds < nds) {
            const uint8_t* rowp = img + t * 16 * kDsRowB;
            const uint4 a0 = *(const uint4*)(rowp + (((dl * 8 + g * 2) ^ n) << 4));
            const uint4 a1 = *(const uint4*)(rowp + (((dl * 8 + g * 2 + 1) ^ n) << 4));
            acc[t] = mfc::mfma16<DT>(a0, bq[2 * ds], acc[t]);
            acc[t] = mfc::mfma16<DT>(a1, bq[2 * ds + 1], acc[t]);
          }
        }
      }
      if (more) store_stage(pf, slot ^ 1, ncs);
      if (wrap) bits_next = __ballot(live_next);
      __syncthreads();  // the other slot is filled, and every wave is done reading this one
      slot ^= 1;
    }

    // ---- epilogue: acc[t][i] = question q against ordinal ob + 16 t + 4 g + i
    const int ob = o_lo + rnd * kDsRound;
#pragma unroll
    for (int t = 0; t < kDsTiles; ++t) {
      if (a.narrow && t != wave) continue;
      const uint32_t nb = (uint32_t)(bits >> (16 * t + 4 * g)) & 15u;
      const int o0 = ob + 16 * t + 4 * g;
      if (!a.thresh) {
        if (qlive && o0 < o_hi) {
          uint64_t key[4];
#pragma unroll
          for (int i = 0; i < 4; ++i)
            key[i] = ((nb >> i) & 1u) && acc[t][i] == acc[t][i] ? cand_key(acc[t][i], (o0 + i) * a.stride) : 0ull;
          uint64_t* dst = a.slab + (int64_t)q * a.slab_stride + o0;  // 16-B aligned: the stride is even, o0 % 4 == 0
          if (o0 + 3 < o_hi) {
            ((u64x2*)dst)[0] = u64x2{key[0], key[1]};
            ((u64x2*)dst)[1] = u64x2{key[2], key[3]};
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (o0 + i < o_hi) dst[i] = key[i];
          }
        }
      } else {
        bool p[4], any = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          p[i] = qlive && ((nb >> i) & 1u) && acc[t][i] >= thr;  // NaN (a tombstoned row) never passes
          any |= p[i];
        }
        if (!__ballot(any)) continue;  // nearly every tile
        // One global atomic per passing row, no aggregation: with tau from the sample about k / S of the rows
        // pass (k = 100 of S = 50k at 10M rows: 0.2 %; k = 1,000 of S = 143k: 0.7 %), a few per wave and round.
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (p[i]) {
            const int at = atomicAdd(a.count + q, 1);
            if (at < a.cap) a.slab[(int64_t)q * a.slab_stride + at] = cand_key(acc[t][i], o0 + i);
          }
      }
    }
    bits = bits_next;
  }
}

// ---- between the passes -------------------------------------------------------------------------------------
// tau[q] = the k-th score the selection found in the sample (-inf: fewer than k eligible sample rows, "none")
__global__ void ds_tau_kernel(const float* __restrict__ sel_s, int k, int nq, float* __restrict__ tau, int* __restrict__ count) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  tau[q] = sel_s[(int64_t)q * k + k - 1];
  count[q] = 0;
}

// One workgroup of 1,024 threads (nq <= 1,024).  n_keys[q] = the slab's keys: n_dense after a DENSE pass, else
// min(count, cap); a question whose count passed cap falls back: fb_list = those questions in ascending order,
// head[0] = their number.
__global__ __launch_bounds__(1024) void ds_close_kernel(const int* __restrict__ count, int nq, int cap, int dense, int n_dense,
                                                        int* __restrict__ n_keys, int* __restrict__ fb_list,
                                                        int* __restrict__ head) {
  __shared__ int wsum[16];
  const int q = threadIdx.x, lane = q & 63, w = q >> 6;
  const int cnt = q < nq ? (dense ? n_dense : count[q]) : 0;
  const bool fell = !dense && cnt > cap;
  if (q < nq) n_keys[q] = min(cnt, cap);
  const uint64_t m = __ballot(fell);
  if (lane == 0) wsum[w] = __popcll(m);
  __syncthreads();
  int base = 0, total = 0;
  for (int i = 0; i < 16; ++i) {
    base += i < w ? wsum[i] : 0;
    total += wsum[i];
  }
  if (fell) fb_list[base + __popcll(m & ((1ull << lane) - 1))] = q;
  if (q == 0) head[0] = total;
}

// The score rule of every search on the selected rows: fl32 of the f64 dot of the stored values, 8 lanes per
// row (rescore_dot).  Block = question; sel_r < 0: no row.
__global__ __launch_bounds__(256) void ds_rescore_kernel(const void* __restrict__ X, int nrows, int D, int dtype,
                                                         const void* __restrict__ Q, const int64_t* __restrict__ sel_r, int k,
                                                         float* __restrict__ rs_s) {
  const int64_t q = blockIdx.x;
  const int gl = threadIdx.x & 7;
  for (int e0 = 0; e0 < k; e0 += 32) {  // (uniform trip count: the shuffles)
    const int e = e0 + (threadIdx.x >> 3);
    int64_t row = e < k ? sel_r[q * k + e] : -1;
    if (row >= nrows) row = -1;
    const double acc = rescore_dot(X, row, Q, q, D, dtype, gl, row >= 0);
    if (gl == 0 && e < k) rs_s[q * k + e] = row >= 0 ? (float)acc : -__builtin_inff();
  }
}

// ---- fallback -----------------------------------------------------------------------------------------------
// block j < head[0]: question fb_list[j] into place j of the compact question buffer (16-B vectors)
__global__ void ds_gather_kernel(const uint4* __restrict__ Q, int vecs, const int* __restrict__ fb_list,
                                 const int* __restrict__ head, uint4* __restrict__ fb_q) {
  const int j = blockIdx.x;
  if (j >= head[0]) return;
  const int64_t q = fb_list[j];
  for (int i = threadIdx.x; i < vecs; i += blockDim.x) fb_q[(int64_t)j * vecs + i] = Q[q * vecs + i];
}
// block j < head[0]: the deep search's answer j over the outputs of question fb_list[j]
__global__ void ds_scatter_kernel(const float* __restrict__ fb_s, const int64_t* __restrict__ fb_r, int k,
                                  const int* __restrict__ fb_list, const int* __restrict__ head, float* __restrict__ out_s,
                                  int64_t* __restrict__ out_r) {
  const int j = blockIdx.x;
  if (j >= head[0]) return;
  const int64_t q = fb_list[j];
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    out_s[q * k + i] = fb_s[(int64_t)j * k + i];
    out_r[q * k + i] = fb_r[(int64_t)j * k + i];
  }
}

template <int DT, int NDS>
void launch_scan_w(const DsScan& a, int q_per_wg, dim3 grid, hipStream_t st) {
  if constexpr (NDS <= 12)  // (the 8-wave form is not built for dim > 768)
    if (q_per_wg == 128) {
      hipLaunchKernelGGL((deep_sampled_scan_kernel<DT, NDS, 8>), grid, dim3(512), 0, st, a);
      return;
    }
  hipLaunchKernelGGL((deep_sampled_scan_kernel<DT, NDS, 4>), grid, dim3(256), 0, st, a);
}
template <int DT>
int launch_scan_dt(const DsScan& a, int q_per_wg, dim3 grid, hipStream_t st) {
  switch ((a.D / 64 + 3) / 4) {
    case 1: launch_scan_w<DT, 4>(a, q_per_wg, grid, st); return 0;
    case 2: launch_scan_w<DT, 8>(a, q_per_wg, grid, st); return 0;
    case 3: launch_scan_w<DT, 12>(a, q_per_wg, grid, st); return 0;
    case 4: launch_scan_w<DT, 16>(a, q_per_wg, grid, st); return 0;
  }
  return -1;
}
// one pass over n_ord ordinals; BOTH passes of a call come through here with the same dtype, D and q_per_wg
int launch_scan(DsScan a, int dtype, const DeepSampledPlan& p, hipStream_t st) {
  int ranges = 0;
  deep_sampled_split(a.n_ord, p.q_groups, &a.ord_per_range, &ranges);
  a.narrow = p.q_per_wg == kDsNarrowQ;
  const dim3 grid((unsigned)ranges, (unsigned)p.q_groups);
  return dtype == RFX_BF16 ? launch_scan_dt<RFX_BF16>(a, p.q_per_wg, grid, st) : launch_scan_dt<RFX_F16>(a, p.q_per_wg, grid, st);
}

}  // namespace

int launch_deep_sampled_search(const DeepSampledPlan& p, const void* X, int64_t nrows, int D, int dtype, const void* Q,
                               int64_t nq, int k, const uint32_t* mask, uint8_t* ws, float* out_s, int64_t* out_r,
                               hipStream_t st) {
  if (dtype != RFX_BF16 && dtype != RFX_F16) return -1;
  if (D < 64 || D > kDeepMaxDim || D % 64 != 0) return -1;
  if (nq < 1 || nq > kDeepMaxNq || k < kDeepMinK || k > p.kb || nrows < 0 || nrows > 0x7fffffffll - 1) return -1;
  if (p.q_per_wg != kDsNarrowQ && p.q_per_wg != 64 && !(p.q_per_wg == 128 && D <= kDsWideMaxDim)) return -1;
  if ((p.cap & 1) || (p.slab & 1) || p.slab < p.cap || ((uintptr_t)ws & 255)) return -1;
  if (p.dense ? p.cap < nrows : (p.S < 1 || p.stride < 1 || (int64_t)(p.S - 1) * p.stride >= nrows || p.slab < p.S)) return -1;
  const DeepSampledWs w = deep_sampled_ws(p, nrows, D, nq, k);
  int* head = (int*)ws;
  int *count = (int*)(ws + w.count), *n_keys = (int*)(ws + w.n_keys), *fb_list = (int*)(ws + w.fb_list);
  float *tau = (float*)(ws + w.tau), *sel_s = (float*)(ws + w.sel_s), *rs_s = (float*)(ws + w.rs_s);
  int64_t* sel_r = (int64_t*)(ws + w.sel_r);
  uint64_t* slab = (uint64_t*)(ws + w.slab);
  const int nqi = (int)nq;

  DsScan a{};
  a.X = (const uint8_t*)X, a.Q = (const uint8_t*)Q, a.mask = mask, a.tau = tau, a.count = count, a.slab = slab;
  a.slab_stride = p.slab, a.D = D, a.nq = nqi, a.cap = p.cap;
  if (!p.dense) {
    // 1. the sample: every sample row's key, the k best of them, tau = the k-th score
    a.n_ord = p.S, a.stride = p.stride, a.thresh = 0;
    if (launch_scan(a, dtype, p, st)) return -1;
    hipLaunchKernelGGL(ds_close_kernel, dim3(1), dim3(1024), 0, st, count, nqi, p.S, 1, p.S, n_keys, fb_list, head);
    if (launch_deep_select(slab, p.slab, n_keys, nq, k, sel_s, sel_r, st)) return -1;
    hipLaunchKernelGGL(ds_tau_kernel, dim3((unsigned)((nqi + 255) / 256)), dim3(256), 0, st, sel_s, k, nqi, tau, count);
  }
  // 2. the main pass over every row
  a.n_ord = (int)nrows, a.stride = 1, a.thresh = p.dense ? 0 : 1;
  if (nrows > 0 && launch_scan(a, dtype, p, st)) return -1;
  hipLaunchKernelGGL(ds_close_kernel, dim3(1), dim3(1024), 0, st, count, nqi, p.cap, p.dense, (int)nrows, n_keys, fb_list, head);
  // 3. the k best by (MFMA score desc, row asc), re-scored by the score rule, ordered again
  if (launch_deep_select(slab, p.slab, n_keys, nq, k, sel_s, sel_r, st)) return -1;
  hipLaunchKernelGGL(ds_rescore_kernel, dim3((unsigned)nq), dim3(256), 0, st, X, (int)nrows, D, dtype, Q, sel_r, k, rs_s);
  if (launch_deep_order(rs_s, sel_r, nq, k, k, out_s, out_r, st)) return -1;
  if (p.dense) return 0;  // a DENSE pass cannot overflow
  // 4. the questions whose slab overflowed: the deep search of k_deep.h over a compact copy, scattered back
  uint4* fb_q = (uint4*)(ws + w.fb_q);
  float* fb_s = (float*)(ws + w.fb_s);
  int64_t* fb_r = (int64_t*)(ws + w.fb_r);
  hipLaunchKernelGGL(ds_gather_kernel, dim3((unsigned)nq), dim3(128), 0, st, (const uint4*)Q, D / 8, fb_list, head, fb_q);
  if (launch_deep_search(deep_plan(nrows, nq, k), X, nrows, D, dtype, fb_q, nq, k, mask, (uint64_t*)(ws + w.parent), fb_s, fb_r,
                         st, head))
    return -1;
  hipLaunchKernelGGL(ds_scatter_kernel, dim3((unsigned)nq), dim3(256), 0, st, fb_s, fb_r, k, fb_list, head, out_s, out_r);
  return 0;
}

}  // namespace rfx
