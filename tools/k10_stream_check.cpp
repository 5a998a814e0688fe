// k10_stream_check.cpp — stand-alone host check of kernel 10's running stream state (csrc/k10_stream.h): no
// device, no HIP.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I rag-foundation_amd/csrc tools/k10_stream_check.cpp -o /tmp/k10_stream_check && /tmp/k10_stream_check
// For every block of a plan it walks the pieces in the order the kernel issues them (the prologue's AHEAD
// stages by the closed form, then one stage per loop step from the cursor) and compares, piece by piece, the
// running source offset, ring slot, record offset and record slot with the closed forms
//   source = tile_of(ti) * 32 * D + si * 256,  slot = h % RING,  record = tile_of(ti) * 16 -> slot ti % 8
// (h the stage index, ti = h / NST, si = h % NST, tile_of(ti) = tb0 + ti * tstride), and the read side's
// slot positions with g % RING and (g + 1) % RING.  The 10M x 768 plan puts the offsets past 2^32.  In the
// tail (h >= S, duplicate loads whose slots are never read) the source must be a stage of the block's last
// tile and the record the last tile's, in the slot it already has.
// The walk below repeats the order of the kernel's issue_run (advance the cursor at si == 0, one ring step per
// stage) and does not share that lambda, which ends in inline asm: it verifies the helpers of k10_stream.h
// and this order, not the kernel's text; tests/test_gpu_screen_lean.py covers the kernel's use of them.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "k10_stream.h"

using namespace rfx::k10s;

static long g_fail = 0;
#define CHECK(c)                                                              \
  do {                                                                        \
    if (!(c)) {                                                               \
      if (g_fail < 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                               \
    }                                                                         \
  } while (0)

struct Split {
  int tb0, tstride, nt;
};

// the kernel's split of the tiles over the blocks (k_scan_screen.h): static, or XCD-balanced by weights
static Split split(int range, int nblk, int ntiles, const uint32_t* xw) {
  Split s{range, nblk, range < ntiles ? (ntiles - range + nblk - 1) / nblk : 0};
  if (xw && (nblk & 7) == 0 && ntiles >= 64 * nblk) {
    const int xc = range & 7;
    uint64_t pre = 0, tot = 0;
    uint32_t wx = 1;
    for (int x = 0; x < 8; ++x) {
      pre += x < xc ? xw[x] : 0u;
      wx = x == xc ? xw[x] : wx;
      tot += xw[x];
    }
    const int t_lo = (int)((uint64_t)ntiles * pre / tot), t_hi = (int)((uint64_t)ntiles * (pre + wx) / tot);
    const int bpx = nblk >> 3;
    s.tb0 = t_lo + (range >> 3);
    s.tstride = bpx;
    s.nt = s.tb0 < t_hi ? (t_hi - s.tb0 + bpx - 1) / bpx : 0;
  }
  return s;
}

static long walk(int64_t rows, int D, int nblk, int RING, int AHEAD, const uint32_t* xw) {
  const int ntiles = (int)((rows + kTileRows - 1) / kTileRows);
  const int NST = D / kStageB;
  const uint64_t total = (uint64_t)ntiles * kTileRows * D;
  const uint32_t slot_b = kTileRows * kStageB, ring_b = (uint32_t)RING * slot_b;
  long pieces = 0;
  int64_t covered = 0;
  for (int b = 0; b < nblk; ++b) {
    const Split sp = split(b, nblk, ntiles, xw);
    covered += sp.nt;
    if (sp.nt == 0) continue;
    const int64_t S = (int64_t)sp.nt * NST;
    auto tile_of = [&](int64_t ti) { return (int64_t)sp.tb0 + ti * sp.tstride; };
    const int t0 = (AHEAD - 1) / NST < sp.nt - 1 ? (AHEAD - 1) / NST : sp.nt - 1;
    TileCursor cur = cursor_at(t0, sp.tb0, sp.tstride, D);
    CHECK(cur.code_byte == (uint64_t)tile_of(t0) * kTileRows * D);
    uint32_t wr = (uint32_t)(AHEAD % RING) * slot_b;
    uint32_t rd = 0, rdn = RING > 1 ? slot_b : 0;
    for (int64_t it = 0; it < sp.nt; ++it)
      for (int s = 0; s < NST; ++s) {
        const int64_t g = it * NST + s, h = g + AHEAD;
        const int si = (int)((s + AHEAD) % NST);
        CHECK(si == (int)(h % NST));
        if (si == 0) cursor_next_tile(cur, sp.nt, sp.tstride, D);
        const int64_t hc = h < S ? h : S - 1, ti = hc / NST;
        const uint64_t src = cur.code_byte + (uint64_t)si * kStageB;
        if (h < S) {
          CHECK(src == (uint64_t)tile_of(ti) * kTileRows * D + (uint64_t)(hc % NST) * kStageB);
        } else {
          CHECK(cur.ti == sp.nt - 1 && cur.code_byte == (uint64_t)tile_of(sp.nt - 1) * kTileRows * D);
        }
        CHECK(cur.ti == (int)ti);
        // the farthest byte a lane of the piece reads: row 31 of the tile, the stage's last 16-B chunk
        CHECK(src + (uint64_t)(kTileRows - 1) * D + kStageB <= total);
        // what a lane adds to the descriptor's base stays within 32 bits
        CHECK((uint64_t)(kTileRows - 1) * D + (uint64_t)(NST - 1) * kStageB + kStageB < (1ull << 32));
        CHECK(wr == (uint32_t)(h % RING) * slot_b);
        if (si == 0) {
          CHECK(cur.rec_byte == (uint32_t)tile_of(ti) * 16u);
          CHECK(cur.mslot == (uint32_t)(ti % kMetaSlots));
        }
        wr = ring_next(wr, slot_b, ring_b);
        CHECK(rd == (uint32_t)(g % RING) * slot_b && rdn == (uint32_t)((g + 1) % RING) * slot_b);
        rd = rdn;
        rdn = ring_next(rdn, slot_b, ring_b);
        ++pieces;
      }
  }
  CHECK(covered == ntiles);
  return pieces;
}

int main() {
  const uint32_t even[8] = {1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024};
  const uint32_t skew[8] = {512, 2048, 1000, 1100, 900, 1024, 2048, 513};
  long n = 0;
  // config 3: 10M x 768, 256 blocks, the 10-slot ring with one barrier per tile (AHEAD = RING - NST)
  n += walk(10'000'000, 768, 256, 10, 7, nullptr);
  n += walk(10'000'000, 768, 256, 10, 7, even);
  n += walk(10'000'000, 768, 256, 10, 7, skew);
  std::printf("10M x 768: last code byte %llu (2^32 = %llu)\n", 10'000'000ull * 768, 1ull << 32);
  // the 2-wave kernel's rings (768: 8 slots per tile barrier; 1024: 8 slots, one barrier per stage), d 1024
  n += walk(10'000'000, 1024, 256, 10, 6, skew);
  n += walk(1'250'000, 768, 512, 8, 5, even);
  n += walk(1'250'000, 1024, 512, 8, 7, skew);
  // short blocks: fewer tiles than the ring, than AHEAD stages, one tile, odd counts, blocks without tiles
  for (int64_t rows = 1; rows <= 32 * 40; rows += 31)
    for (int nblk : {1, 3, 8}) {
      n += walk(rows, 768, nblk, 10, 7, nullptr);
      n += walk(rows, 768, nblk, 8, 5, nullptr);
      n += walk(rows, 1024, nblk, 8, 7, nullptr);
      n += walk(rows, 1024, nblk, 10, 6, nullptr);
    }
  for (int64_t rows : {(int64_t)64 * 8 * 32, (int64_t)64 * 8 * 32 + 1, (int64_t)65'536, (int64_t)60'000})
    for (int nblk : {8, 16}) n += walk(rows, 768, nblk, 10, 7, skew);
  std::printf("%ld pieces walked, %ld failures\n", n, g_fail);
  return g_fail ? 1 : 0;
}
