// k_compact.h — store compaction: gather the kept rows of an index into a fresh allocation.
//
// Path: delete_document_from_store (gemini_rag.py:392-424) leaves NaN rows behind; rfx_index_compact copies
// the rows that are kept, in order, into a new buffer and frees the old one.  Host plan: compact_plan.h.
//
// Destination row p (a POSITION among the kept rows) is source row row0[i] + (p - pos0[i]) of the range i
// that holds p.  One launch for any number of ranges: a workgroup (4 waves) owns one chunk of positions
// [pos0, pos0 + n), which may span many ranges, and treats it as n * VPR 16-byte vectors (VPR = row bytes /
// 16; row bytes are a multiple of 128).  Thread t moves vectors t, t + 256, ...: four 16-B loads in flight
// per lane, then four 16-B stores, so a wave's accesses are 1-KiB runs on both sides whatever the row
// length.  The kernel moves bits: any dtype, and a kept row that is tombstoned stays NaN.
//
// A lane finds the range of a position through the table, starting from the range it last used (its
// positions only grow): a galloping probe, then a binary search — one or two table reads when the next
// position lies in the next range, log2(ranges) at worst.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "compact_plan.h"

namespace rfx {

constexpr int kCompactThreads = 256;
constexpr int kCompactUnroll = 4;

// Gathers `kept` rows of `vpr` 16-byte vectors each from src (nrows rows) into dst (at least kept rows).
// Returns 0, or -1 for arguments it refuses (nothing launched).
int launch_compact_rows(const void* src, int64_t nrows, void* dst, int64_t kept, int64_t row_bytes,
                        const CompactChunkDev* chunks_d, int n_chunks, const CompactRangeDev* ranges_d, int n_ranges,
                        hipStream_t st);

}  // namespace rfx
