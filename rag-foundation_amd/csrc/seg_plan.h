// seg_plan.h — host-only: validation and work list of the segmented search (rfx_search_segmented,
// rfx_segmented_plan; kernel: k_scan_seg.h).  Plain C++ (no HIP): the library includes it, and so can a
// stand-alone host program (sanitizer runs of the plan need no device).
//
// Path: a batch of questions under DIFFERENT metadata filters (the file-search tool's metadata_filter,
// gemini_rag.py:463-469, allow-listed per tenant / user at chat.py:295-335) answered by ONE scan that
// reads only the rows each filter selects.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

namespace rfx {

constexpr int kSegLists = 64;        // L: a group's selected rows are cut into at most L chunks
constexpr int kSegMinChunk = 128;    // rows: a workgroup's least share (32 rows per wave)
constexpr int kSegChunkAlign = 64;   // a chunk is a multiple of 4 waves x 16 rows (the last one excepted)
constexpr int kSegSlice = 8;         // queries per work item
constexpr int64_t kSegMaxNq = 1024;  // queries per call (the batcher's max_batch is 256)

// One work item, as rfx_segmented_plan reports it ([4] int64: group, first query, first selected-row
// position, selected rows) plus what the kernel needs beside it.
struct SegItem {
  int64_t group, q0, pos0, n;
  int nqt;           // queries of the slice (1..8)
  int list;          // the chunk's number in its group: the candidate list the item writes
  int64_t r_lo;      // index (into the call's range table) of the range that holds position pos0
  int64_t r_hi;      // end of the group's ranges
};

// Device tables (uploaded into the workspace).  Positions count a group's selected rows in range order.
struct SegItemDev {  // 32 B
  int q0, nqt, r_lo, r_hi, pos0, n, list, pad;
};
struct SegRangeDev {  // 16 B: rows row0 + (p - pos0) for positions p in [pos0, pos1)
  int row0, pos0, pos1, pad;
};

inline int64_t seg_chunk_rows(int64_t rows_g) {
  int64_t c = std::max<int64_t>(kSegMinChunk, (rows_g + kSegLists - 1) / kSegLists);
  return (c + kSegChunkAlign - 1) / kSegChunkAlign * kSegChunkAlign;
}

// Upper bound of the work items of any valid call with nq queries (workspace sizing): every slice holds
// at least one query and is cut into at most L chunks.
inline int64_t seg_max_items(int64_t nq) { return nq * kSegLists; }

// Returns "" when the arguments describe a valid call, else what is wrong with them.  Nothing is read
// past the lengths the arguments themselves give: group arrays n_groups + 1, ranges 2 * group_r[n_groups].
inline std::string seg_validate(int64_t rows, int64_t nq, int k, int n_groups, const int64_t* gq, const int64_t* gr,
                                const int64_t* ranges) {
  if (rows < 0 || rows > 0x7fffffffll - 1) return "rows out of [0, 2^31 - 2]";
  if (k < 1 || k > 64) return "k out of [1, 64]";
  if (nq < 0 || nq > kSegMaxNq) return "nq out of [0, " + std::to_string(kSegMaxNq) + "]";
  if (n_groups < 0) return "n_groups < 0";
  if (n_groups == 0) return nq == 0 ? "" : "queries without a group";
  if (!gq || !gr) return "null group arrays";
  if (gq[0] != 0 || gr[0] != 0) return "group arrays must start at 0";
  for (int g = 0; g < n_groups; ++g) {
    if (gq[g + 1] < gq[g]) return "group_q not monotone at group " + std::to_string(g);
    if (gr[g + 1] < gr[g]) return "group_r not monotone at group " + std::to_string(g);
    if (gq[g + 1] > nq) return "group_q exceeds nq at group " + std::to_string(g);
  }
  if (gq[n_groups] != nq) return "group_q[n_groups] != nq";
  if (gr[n_groups] > 0 && !ranges) return "null ranges";
  for (int g = 0; g < n_groups; ++g) {
    int64_t end = 0;  // first row past the previous range of the group
    for (int64_t i = gr[g]; i < gr[g + 1]; ++i) {
      const int64_t first = ranges[2 * i], count = ranges[2 * i + 1];
      const std::string at = " (group " + std::to_string(g) + ", range " + std::to_string(i - gr[g]) + ")";
      if (count <= 0) return "range count <= 0" + at;
      if (first < 0 || first >= rows || count > rows - first) return "range outside [0, rows)" + at;
      if (first < end) return "ranges unsorted or overlapping" + at;
      end = first + count;
    }
  }
  return "";
}

// The work list of a VALID call (seg_validate passed), heaviest items first (a stable order: among equal
// sizes group, slice, chunk ascending), and the candidate lists per query the call needs (<= L, >= 1).
inline int seg_plan(int64_t nq, int n_groups, const int64_t* gq, const int64_t* gr, const int64_t* ranges,
                    std::vector<SegItem>& items) {
  items.clear();
  int lists = 1;
  for (int g = 0; g < n_groups; ++g) {
    const int64_t q_lo = gq[g], q_hi = gq[g + 1], r_lo = gr[g], r_hi = gr[g + 1];
    int64_t rows_g = 0;
    for (int64_t i = r_lo; i < r_hi; ++i) rows_g += ranges[2 * i + 1];
    if (q_hi == q_lo || rows_g == 0) continue;
    const int64_t chunk = seg_chunk_rows(rows_g);
    const int n_chunks = (int)((rows_g + chunk - 1) / chunk);
    lists = std::max(lists, n_chunks);
    for (int64_t q0 = q_lo; q0 < q_hi; q0 += kSegSlice) {
      int64_t ri = r_lo, r_pos = 0;  // range ri starts at position r_pos
      for (int c = 0; c < n_chunks; ++c) {
        const int64_t pos0 = (int64_t)c * chunk;
        while (pos0 >= r_pos + ranges[2 * ri + 1]) r_pos += ranges[2 * ri++ + 1];
        SegItem it;
        it.group = g;
        it.q0 = q0;
        it.pos0 = pos0;
        it.n = std::min(chunk, rows_g - pos0);
        it.nqt = (int)std::min<int64_t>(kSegSlice, q_hi - q0);
        it.list = c;
        it.r_lo = ri;
        it.r_hi = r_hi;
        items.push_back(it);
      }
    }
  }
  std::stable_sort(items.begin(), items.end(), [](const SegItem& a, const SegItem& b) { return a.n > b.n; });
  return lists;
}

// The range table of a valid call: per range its first row and its positions within its group.
inline void seg_ranges_dev(int n_groups, const int64_t* gr, const int64_t* ranges, SegRangeDev* out) {
  for (int g = 0; g < n_groups; ++g) {
    int64_t pos = 0;
    for (int64_t i = gr[g]; i < gr[g + 1]; ++i) {
      out[i] = SegRangeDev{(int)ranges[2 * i], (int)pos, (int)(pos + ranges[2 * i + 1]), 0};
      pos += ranges[2 * i + 1];
    }
  }
}

inline SegItemDev seg_item_dev(const SegItem& it) {
  return SegItemDev{(int)it.q0, it.nqt, (int)it.r_lo, (int)it.r_hi, (int)it.pos0, (int)it.n, it.list, 0};
}

}  // namespace rfx
