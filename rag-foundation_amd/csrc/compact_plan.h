// compact_plan.h — host-only: validation, range table and work split of the store compaction
// (rfx_index_compact, rfx_compact_plan; kernel: k_compact.h).  Plain C++ (no HIP): the library includes it,
// and so can a stand-alone host program (sanitizer runs of the plan need no device).
//
// Path: delete_document_from_store (gemini_rag.py:392-424) tombstones a document's rows; compaction gathers
// the rows that are KEPT into a fresh allocation so the deleted ones stop costing memory and scan bytes.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

namespace rfx {

constexpr int kCompactMaxChunks = 4096;   // work chunks of a call, however many ranges it has
constexpr int kCompactMinChunk = 32;      // rows: a workgroup's least share
constexpr int kCompactChunkAlign = 32;    // a chunk is a multiple of this (the last one excepted)

// Device tables.  Positions count the kept rows in range order: destination row p IS position p.
struct CompactRangeDev {  // 16 B: source rows row0 + (p - pos0) for positions p in [pos0, pos1)
  int row0, pos0, pos1, pad;
};
struct CompactChunkDev {  // 16 B: positions [pos0, pos0 + n); r_lo = the range that holds pos0
  int pos0, n, r_lo, pad;
};

// Returns "" when `ranges` ([n_ranges][2] = first, count) are valid keep ranges of an index of `rows` rows:
// ascending, disjoint, count > 0, inside [0, rows).  Nothing is read past 2 * n_ranges values.
inline std::string compact_validate(int64_t rows, const int64_t* ranges, int64_t n_ranges) {
  if (rows < 0 || rows > 0x7fffffffll - 1) return "rows out of [0, 2^31 - 2]";
  if (n_ranges < 0 || n_ranges > rows) return "n_ranges out of [0, rows]";
  if (n_ranges > 0 && !ranges) return "null ranges";
  int64_t end = 0;  // first row past the previous range
  for (int64_t i = 0; i < n_ranges; ++i) {
    const int64_t first = ranges[2 * i], count = ranges[2 * i + 1];
    const std::string at = " (range " + std::to_string(i) + ")";
    if (count <= 0) return "range count <= 0" + at;
    if (first < 0 || first >= rows || count > rows - first) return "range outside [0, rows)" + at;
    if (first < end) return "ranges unsorted or overlapping" + at;
    end = first + count;
  }
  return "";
}

inline int64_t compact_chunk_rows(int64_t kept) {
  const int64_t c = std::max<int64_t>(kCompactMinChunk, (kept + kCompactMaxChunks - 1) / kCompactMaxChunks);
  return (c + kCompactChunkAlign - 1) / kCompactChunkAlign * kCompactChunkAlign;
}

// The tables of VALID ranges (compact_validate passed).  Returns the kept rows.  The chunks tile the
// positions [0, kept) exactly once, in order; there are at most kCompactMaxChunks of them.
inline int64_t compact_plan(const int64_t* ranges, int64_t n_ranges, std::vector<CompactRangeDev>& table,
                            std::vector<CompactChunkDev>& chunks) {
  table.clear();
  chunks.clear();
  table.reserve((size_t)n_ranges);
  int64_t pos = 0;
  for (int64_t i = 0; i < n_ranges; ++i) {
    table.push_back(CompactRangeDev{(int)ranges[2 * i], (int)pos, (int)(pos + ranges[2 * i + 1]), 0});
    pos += ranges[2 * i + 1];
  }
  const int64_t kept = pos;
  if (kept == 0) return 0;
  const int64_t chunk = compact_chunk_rows(kept);
  int64_t ri = 0;
  for (int64_t p0 = 0; p0 < kept; p0 += chunk) {
    while (p0 >= table[(size_t)ri].pos1) ++ri;
    chunks.push_back(CompactChunkDev{(int)p0, (int)std::min(chunk, kept - p0), (int)ri, 0});
  }
  return kept;
}

// Source row of destination position p (0 <= p < kept), as the kernel finds it: the range whose pos1 > p.
inline int64_t compact_source_row(const std::vector<CompactRangeDev>& table, int64_t p) {
  size_t lo = 0, hi = table.size() - 1;
  while (lo < hi) {
    const size_t mid = (lo + hi) >> 1;
    if (table[mid].pos1 > p)
      hi = mid;
    else
      lo = mid + 1;
  }
  return (int64_t)table[lo].row0 + (p - table[lo].pos0);
}

}  // namespace rfx
