// k_scan_seg.h — the segmented scan: an exact VALU scan + per-query top-k over a WORK LIST, so one launch
// serves questions under different metadata filters and reads only the rows each filter selects.
// Instantiated per index dtype in seg_f32.hip, seg_bf16.hip and seg_f16.hip; the launcher and the
// candidate fill are in k_scan_seg.hip, the host's work list in seg_plan.h.
//
// Path: the retrieval half of GeminiRag.ask_stream (gemini_rag.py:517-551) under the file-search tool's
// metadata_filter (gemini_rag.py:463-469; allow-listed per tenant / user at chat.py:295-335).
//
// A work item (one workgroup of 4 waves) = up to 8 queries of one filter group x one chunk of the group's
// selected rows.  A chunk is an interval [pos0, pos0 + n) of POSITIONS: the group's (first, count) ranges
// laid end to end; it may span several ranges.  Each lane maps its position to a row through the range
// table (a binary search from the range it last used: no load while it stays inside that range), the row
// stream is scan_valu_body's (k_scan_valu.h): one row per 16-lane group and iteration, read once in 16-B
// lanes for all the slice's queries (widened exactly to f32 in LDS), three iterations in flight, per-wave
// sorted lists merged per block into list `item.list` of each query: cand [nq][n_lists][K].
// Algorithmic bytes: D * esz per selected row and slice.
#pragma once
#include "k_scan_valu.h"
#include "seg_plan.h"

namespace rfx {

template <int DT, int K, int VPL>
__global__ __launch_bounds__(256) void scan_seg_kernel(const uint8_t* __restrict__ X, int nrows, int D,
                                                       const void* __restrict__ Q,
                                                       const SegItemDev* __restrict__ items,
                                                       const SegRangeDev* __restrict__ R,
                                                       float* __restrict__ cand_s, int* __restrict__ cand_r,
                                                       int n_lists) {
  constexpr int NQT = kSegSlice;
  constexpr int ESZ = DT == RFX_F32 ? 4 : 2;
  constexpr int EPV = 16 / ESZ;
  extern __shared__ __attribute__((aligned(16))) float q_lds[];  // [NQT][D]
  const int tid = threadIdx.x;
  const int lane = tid & 63, g = lane >> 4, j = lane & 15, w = tid >> 6;
  const SegItemDev item = items[blockIdx.x];
  const int q0 = item.q0;
  const int nqt = __builtin_amdgcn_readfirstlane(item.nqt);  // wave-uniform: the unused query slots cost a branch
  const int r_hi = item.r_hi;
  const int VPR = D * ESZ / 16;
  const int64_t RB = (int64_t)D * ESZ;
  // the wave's positions [wb, we): a quarter of the chunk, a multiple of 4
  const int rpw = ((item.n + 3) / 4 + 3) & ~3;
  const int wb = item.pos0 + min(w * rpw, item.n);
  const int we = item.pos0 + min(w * rpw + rpw, item.n);

  WaveList<K> L[NQT];
#pragma unroll
  for (int qi = 0; qi < NQT; ++qi) L[qi].init();
  float cand[NQT];
#pragma unroll
  for (int qi = 0; qi < NQT; ++qi) cand[qi] = 0.f;

  // position -> row.  The lane keeps the range it last used (ri, rec); positions only grow, so the search
  // starts there.  The host validated every range against nrows; the clamp keeps a damaged table inside X.
  int ri = item.r_lo;
  SegRangeDev rec = R[ri];
  auto row_of = [&](int p) -> int {
    if (p >= rec.pos1) {
      int lo = min(ri + 1, r_hi - 1), hi = r_hi - 1;  // the first range whose pos1 > p
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (R[mid].pos1 > p)
          hi = mid;
        else
          lo = mid + 1;
      }
      ri = lo;
      rec = R[ri];
    }
    return min(max(rec.row0 + (p - rec.pos0), 0), nrows - 1);
  };
  const int T = we > wb ? (we - wb + 15) / 16 * 4 : 0;  // iterations of 4 rows, a multiple of 4
  int first_row = 0, rows_cur = 0, rows_nxt = 0, cur_blk = 0;
  // the rows of 64-position block b: lane (g, j) holds the row of position wb + 64 b + 4 j + g (the row it
  // offers); positions past the wave's end hold the wave's first row (read again, never offered)
  auto blk_rows = [&](int b) -> int {
    const int p = wb + 64 * b + 4 * j + g;
    return p < we ? row_of(p) : first_row;
  };
  if (T > 0) {
    first_row = row_of(wb);
    rows_cur = blk_rows(0);
    rows_nxt = blk_rows(1);
  }

  // iteration t reads the row of position wb + 64 (t >> 4) + 4 (t & 15) + g: lane (g, t & 15)'s of block
  // t >> 4, which is the block being scored or the one after it (the loads run at most 6 iterations ahead)
  auto load_row = [&](int t, uint4 (&v)[VPL]) {
    const int src = (t >> 4) == cur_blk ? rows_cur : rows_nxt;
    const int row = __shfl(src, (lane & 48) | (t & 15));
    const uint8_t* rp = X + (int64_t)row * RB;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int vv = j + 16 * i;
      const uint4 x = *(const uint4*)(rp + (int64_t)(vv < VPR ? vv : VPR - 1) * 16);
      const uint32_t m = vv < VPR ? 0xffffffffu : 0u;  // AND, not a select (k_scan_valu.h)
      v[i] = make_uint4(x.x & m, x.y & m, x.z & m, x.w & m);
    }
  };
  auto score_row = [&](int it, const uint4 (&v)[VPL]) {
#pragma unroll
    for (int qi = 0; qi < NQT; ++qi) {
      if (qi >= nqt) continue;
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        if (16 * i >= VPR) continue;
#pragma unroll
        for (int e = 0; e < EPV; ++e) {
          const float qv = (j + 16 * i < VPR) ? q_lds[qi * D + (j + 16 * i) * EPV + e] : 0.f;
          acc = fmaf(elem<DT>(v[i], e), qv, acc);
        }
      }
      acc = row16_sum(acc);
      if (j == it) cand[qi] = acc;
    }
  };

  uint4 va[VPL], vb[VPL], vc[VPL], vd[VPL];
  if (T > 0) {  // the first rows are in flight while the queries are staged
    load_row(0, va);
    load_row(1, vb);
    load_row(2, vc);
  }
  for (int i = tid; i < nqt * D; i += 256) q_lds[i] = query_elem<DT>(Q, (int64_t)q0 * D + i);
  __syncthreads();

  for (int t = 0; t < T; t += 4) {
    load_row(t + 3, vd);
    score_row(t & 15, va);
    load_row(t + 4, va);
    score_row((t + 1) & 15, vb);
    load_row(t + 5, vb);
    score_row((t + 2) & 15, vc);
    load_row(t + 6, vc);
    score_row((t + 3) & 15, vd);
    if (((t + 4) & 15) == 0 || t + 4 >= T) {  // block done (or the last, partial one): offer it
      const bool ok = wb + 64 * cur_blk + 4 * j + g < we;
#pragma unroll
      for (int qi = 0; qi < NQT; ++qi)
        if (qi < nqt) L[qi].offer(cand[qi], rows_cur, ok);
      if (t + 4 < T) {
        rows_cur = rows_nxt;
        ++cur_blk;
        rows_nxt = blk_rows(cur_blk + 1);
      }
    }
  }

  // block-level merge: the 4 wave lists of a query -> the item's list; wave w merges queries w, w + 4
  __shared__ float ms[4][NQT][K];
  __shared__ int mr[4][NQT][K];
  if (lane < K) {
#pragma unroll
    for (int qi = 0; qi < NQT; ++qi) {
      ms[w][qi][lane] = L[qi].ls;
      mr[w][qi][lane] = L[qi].lr;
    }
  }
  __syncthreads();
  for (int qi = w; qi < nqt; qi += 4) {
    WaveList<K> M;
    M.init();
#pragma unroll
    for (int src = 0; src < 4; ++src) {
      const bool v = lane < K;
      M.offer(v ? ms[src][qi][lane] : -__builtin_inff(), v ? mr[src][qi][lane] : kEmptyRow,
              v && mr[src][qi][lane] != kEmptyRow);
    }
    if (lane < K) {
      const int64_t o = ((int64_t)(q0 + qi) * n_lists + item.list) * K + lane;
      cand_s[o] = M.ls;
      cand_r[o] = M.lr;
    }
  }
}

// One index dtype's launch (instantiated in seg_<dtype>.hip): k_slot 16 or 64, vpl = ceil(D * esz / 256).
template <int DT>
int launch_seg_dt(int k_slot, int vpl, int n_items, size_t lds, hipStream_t st, const uint8_t* X, int nrows, int D,
                  const void* Q, const SegItemDev* items, const SegRangeDev* R, float* cs, int* cr, int n_lists) {
#define RFX_S(KV, V)                                                                                             \
  if (k_slot == KV && vpl <= V) {                                                                                \
    hipLaunchKernelGGL((scan_seg_kernel<DT, KV, V>), dim3((unsigned)n_items), dim3(256), lds, st, X, nrows, D, Q, \
                       items, R, cs, cr, n_lists);                                                               \
    return 0;                                                                                                    \
  }
  RFX_S(16, 4) RFX_S(16, 8) RFX_S(16, 12) RFX_S(16, 16)
  RFX_S(64, 4) RFX_S(64, 8) RFX_S(64, 12) RFX_S(64, 16)
#undef RFX_S
  return -1;
}
#define RFX_SEG_DT_DECL(NAME)                                                                                     \
  int NAME(int k_slot, int vpl, int n_items, size_t lds, hipStream_t st, const uint8_t* X, int nrows, int D,       \
           const void* Q, const SegItemDev* items, const SegRangeDev* R, float* cs, int* cr, int n_lists);
RFX_SEG_DT_DECL(launch_seg_f32)
RFX_SEG_DT_DECL(launch_seg_bf16)
RFX_SEG_DT_DECL(launch_seg_f16)
#undef RFX_SEG_DT_DECL

}  // namespace rfx
