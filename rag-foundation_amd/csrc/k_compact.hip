// k_compact.hip — the gather kernel of the store compaction and its launcher (see k_compact.h).
#include "k_compact.h"

namespace rfx {

__global__ __launch_bounds__(kCompactThreads) void compact_rows_kernel(const uint4* __restrict__ src, int nrows,
                                                                       uint4* __restrict__ dst, int kept, int vpr,
                                                                       const CompactChunkDev* __restrict__ chunks,
                                                                       const CompactRangeDev* __restrict__ R,
                                                                       int n_ranges) {
  const CompactChunkDev c = chunks[blockIdx.x];
  const uint32_t total = (uint32_t)c.n * (uint32_t)vpr;  // <= 2^19 rows x 2^10 vectors (compact_plan.h, dim <= 4096)
  const int r_last = n_ranges - 1;

  // position -> source row.  The host validated every range against nrows; the clamps keep a damaged table
  // inside src and dst.
  int ri = min(max(c.r_lo, 0), r_last);
  CompactRangeDev rec = R[ri];
  auto row_of = [&](int p) -> int {
    if (p >= rec.pos1 && ri < r_last) {
      int lo = ri + 1, step = 1;  // gallop: the first range whose pos1 > p lies in [lo, hi]
      while (ri + step < r_last && R[ri + step].pos1 <= p) {
        lo = ri + step + 1;
        step *= 2;
      }
      int hi = min(ri + step, r_last);
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

  for (uint32_t v0 = threadIdx.x; v0 < total; v0 += kCompactThreads * kCompactUnroll) {
    uint4 x[kCompactUnroll];
    int64_t d[kCompactUnroll];
#pragma unroll
    for (int i = 0; i < kCompactUnroll; ++i) {
      const uint32_t v = v0 + (uint32_t)i * kCompactThreads;
      d[i] = -1;
      if (v < total) {  // (a lane past the chunk's end loads and stores nothing)
        const uint32_t pr = v / (uint32_t)vpr, col = v - pr * (uint32_t)vpr;
        const int p = c.pos0 + (int)pr;
        x[i] = src[(int64_t)row_of(p) * vpr + col];
        if (p < kept) d[i] = (int64_t)p * vpr + col;
      }
    }
#pragma unroll
    for (int i = 0; i < kCompactUnroll; ++i)
      if (d[i] >= 0) dst[d[i]] = x[i];
  }
}

int launch_compact_rows(const void* src, int64_t nrows, void* dst, int64_t kept, int64_t row_bytes,
                        const CompactChunkDev* chunks_d, int n_chunks, const CompactRangeDev* ranges_d, int n_ranges,
                        hipStream_t st) {
  if (kept <= 0 || n_chunks <= 0) return 0;
  if (!src || !dst || !chunks_d || !ranges_d || n_ranges <= 0 || n_chunks > kCompactMaxChunks) return -1;
  if (nrows <= 0 || nrows > 0x7fffffffll - 1 || kept > nrows) return -1;
  if (row_bytes <= 0 || row_bytes % 128 != 0 || row_bytes / 16 > 1024) return -1;
  hipLaunchKernelGGL(compact_rows_kernel, dim3(n_chunks), dim3(kCompactThreads), 0, st, (const uint4*)src, (int)nrows,
                     (uint4*)dst, (int)kept, (int)(row_bytes / 16), chunks_d, ranges_d, n_ranges);
  return 0;
}

}  // namespace rfx
