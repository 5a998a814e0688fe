// index_access.h — what a C-ABI translation unit other than rfx_api.hip (which owns the index handles) may see
// of an index: its geometry and rows, under the index's reader lock.
#pragma once
#include <stdint.h>

#include <memory>
#include <shared_mutex>

#include "../../include/rfx.h"

namespace rfx {

struct IndexRead {
  std::shared_ptr<void> keep;                     // the index stays alive
  std::shared_lock<std::shared_timed_mutex> lk;   // reader lock: no append, tombstone or compaction meanwhile
  int device = 0, dim = 0, dtype = 0;
  int64_t rows = 0;
  const void* data = nullptr;  // [capacity][dim] of dtype; rows past `rows` hold NaN
  bool view = false;           // a union view
};

// RFX_OK with *out filled and the lock held until *out dies; RFX_EINVAL (unknown handle) or RFX_EBUSY (the
// reader lock timed out) with rfx_last_error set.
int api_index_read(rfx_index_t h, IndexRead* out);

// `bytes` of per-question tables to dst_d on stream st through the index's pinned staging buffer, as
// rfx_search_segmented stages its tables: fill(stage, ctx) writes them on the host, the caller's arrays may die on
// return and the copy stays stream-ordered.  RFX_OK, or RFX_ENOMEM / RFX_EDEVICE with rfx_last_error set.
int api_stage_tables(const IndexRead& ix, size_t bytes, void (*fill)(uint8_t* stage, void* ctx), void* ctx, void* dst_d,
                     void* st);

}  // namespace rfx
