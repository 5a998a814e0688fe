// k10_stream.h — kernel 10's corpus stream as running state (round 8): where the next LDS-DMA piece comes
// from and which ring slot it goes to, advanced by one step per stage instead of recomputed from the
// stage index (a modulo by the ring size, a division by the stages per tile, a 64-bit tile address and a
// fresh buffer descriptor per piece).  Plain C++, host-callable: tools/k10_stream_check.cpp walks every
// piece of a 10M-row plan and compares the running values with the closed forms below.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RFX_K10S_HD __host__ __device__ __forceinline__
#else
#define RFX_K10S_HD inline
#endif

namespace rfx {
namespace k10s {

constexpr int kTileRows = 32;   // rows per tile (k10::kTM)
constexpr int kStageB = 256;    // codes (bytes) per row per stage (k10::kSK)
constexpr int kMetaSlots = 8;   // tile-record slots in LDS (k10::kMR)
constexpr int kRecB = 16;       // bytes per tile record

// The tile whose pieces are being issued.  The code array exceeds 2^32 bytes (10M x 768), so the byte
// offset of the tile is 64 bits and becomes the base of the buffer descriptor, rebased once per tile; what
// a piece adds to it (the lane's offset in the tile, < 32 D, and the stage's 256 si) stays far below 2^32.
struct TileCursor {
  uint64_t code_byte;  // byte offset of the tile's first code from the start of the code array
  uint32_t rec_byte;   // byte offset of the tile's record in the record array (tile * 16)
  uint32_t mslot;      // the LDS slot of the record (block-local tile index % kMetaSlots)
  int ti;              // block-local tile index, never past nt - 1
};

// closed form: block-local tile ti of a block whose tiles are tb0 + i * tstride
RFX_K10S_HD TileCursor cursor_at(int ti, int tb0, int tstride, int D) {
  const int64_t tile = (int64_t)tb0 + (int64_t)ti * tstride;
  TileCursor c;
  c.code_byte = (uint64_t)tile * (uint64_t)(kTileRows * D);
  c.rec_byte = (uint32_t)tile * (uint32_t)kRecB;
  c.mslot = (uint32_t)ti % (uint32_t)kMetaSlots;
  c.ti = ti;
  return c;
}

// One tile on, at the first stage of the next tile.  Past the block's last tile the cursor stays where it
// is: the tail's pieces (issued only so that the counted waits stay exact, their slots never read) re-load
// data of the last tile, and its record goes to the slot it already occupies.
RFX_K10S_HD void cursor_next_tile(TileCursor& c, int nt, int tstride, int D) {
  if (c.ti + 1 < nt) {
    ++c.ti;
    c.code_byte += (uint64_t)(uint32_t)tstride * (uint64_t)(kTileRows * D);
    c.rec_byte += (uint32_t)tstride * (uint32_t)kRecB;
    c.mslot = (c.mslot + 1u) & (uint32_t)(kMetaSlots - 1);
  }
}

// a ring position in bytes (slot * slot_bytes), one slot on: compare and select, no modulo
RFX_K10S_HD uint32_t ring_next(uint32_t off, uint32_t slot_bytes, uint32_t ring_bytes) {
  const uint32_t n = off + slot_bytes;
  return n == ring_bytes ? 0u : n;
}

}  // namespace k10s
}  // namespace rfx
