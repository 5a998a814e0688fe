// compact_plan_check.cpp — stand-alone host driver of the store compaction's plan (csrc/compact_plan.h): no
// device, no HIP.  Meant for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I rag-foundation_amd/csrc tools/compact_plan_check.cpp -o /tmp/compact_plan_check && /tmp/compact_plan_check
// It runs the validation over malformed inputs and the plan over hand-made and random valid ones, with the
// ranges in a heap array of the exact length the arguments give (so any read past it is reported), and checks
// that the chunks tile the kept positions exactly once, that their number is bounded, and that the kernel's
// walk (gallop + binary search from the range last used) sends every position to the right source row.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>

#include "compact_plan.h"

using namespace rfx;

static int g_fail = 0;
#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                              \
    }                                                        \
  } while (0)

struct Call {
  int64_t rows, n_ranges;
  std::unique_ptr<int64_t[]> ranges;  // exact length
};

static Call make(int64_t rows, const std::vector<int64_t>& ranges) {
  Call c;
  c.rows = rows;
  c.n_ranges = (int64_t)ranges.size() / 2;
  c.ranges.reset(new int64_t[ranges.size()]);
  std::copy(ranges.begin(), ranges.end(), c.ranges.get());
  return c;
}

static std::string validate(const Call& c) { return compact_validate(c.rows, c.ranges.get(), c.n_ranges); }

// the kernel's position -> row walk (k_compact.hip), over exact-length copies of the tables
static int64_t walk(const CompactRangeDev* R, int n_ranges, int& ri, int p) {
  const int r_last = n_ranges - 1;
  if (p >= R[ri].pos1 && ri < r_last) {
    int lo = ri + 1, step = 1;
    while (ri + step < r_last && R[ri + step].pos1 <= p) {
      lo = ri + step + 1;
      step *= 2;
    }
    int hi = std::min(ri + step, r_last);
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (R[mid].pos1 > p)
        hi = mid;
      else
        lo = mid + 1;
    }
    ri = lo;
  }
  return (int64_t)R[ri].row0 + (p - R[ri].pos0);
}

static void check_plan(const Call& c, int stride = 1) {
  CHECK(validate(c).empty());
  std::vector<CompactRangeDev> table;
  std::vector<CompactChunkDev> chunks;
  const int64_t kept = compact_plan(c.ranges.get(), c.n_ranges, table, chunks);
  std::vector<int64_t> want;  // the source row of every kept position
  for (int64_t i = 0; i < c.n_ranges; ++i)
    for (int64_t r = c.ranges[2 * i]; r < c.ranges[2 * i] + c.ranges[2 * i + 1]; ++r) want.push_back(r);
  CHECK(kept == (int64_t)want.size());
  CHECK((int64_t)table.size() == c.n_ranges);
  CHECK((int64_t)chunks.size() <= kCompactMaxChunks);
  CHECK((kept == 0) == chunks.empty());
  std::unique_ptr<CompactRangeDev[]> R(new CompactRangeDev[table.size()]);
  std::copy(table.begin(), table.end(), R.get());
  int64_t next = 0;
  for (const CompactChunkDev& ch : chunks) {
    CHECK(ch.pos0 == next && ch.n > 0);  // in order, no gap, no overlap
    next = (int64_t)ch.pos0 + ch.n;
    CHECK(ch.r_lo >= 0 && ch.r_lo < (int)table.size());
    CHECK(R[ch.r_lo].pos0 <= ch.pos0 && ch.pos0 < R[ch.r_lo].pos1);
    int ri = ch.r_lo;
    for (int p = ch.pos0; p < ch.pos0 + ch.n; p += stride) {  // a lane's positions only grow
      const int64_t row = walk(R.get(), (int)table.size(), ri, p);
      CHECK(row == want[(size_t)p] && row < c.rows);
      CHECK(compact_source_row(table, p) == row);
    }
  }
  CHECK(next == kept);
}

int main() {
  // hand-made: single rows, 32- and 128-row boundaries, the last row, a run of small ranges, keep-all, keep-none
  check_plan(make(5000, {0, 1, 3, 1, 20, 12, 32, 40, 100, 60, 300, 3, 304, 3, 308, 3, 4990, 10}));
  check_plan(make(5000, {0, 5000}));
  check_plan(make(5000, {}));
  check_plan(make(0, {}));
  check_plan(make(1, {0, 1}));
  check_plan(make(129, {31, 1, 32, 1, 127, 2}));
  {
    std::vector<int64_t> r;  // more ranges than chunks: 300,000 ranges of 1 row
    for (int64_t i = 0; i < 300000; ++i) r.insert(r.end(), {2 * i, 1});
    check_plan(make(600000, r));
    check_plan(make(600000, r), 7);
  }
  // malformed
  CHECK(!validate(make(100, {50, 5, 10, 5})).empty());
  CHECK(!validate(make(100, {10, 5, 14, 5})).empty());
  CHECK(!validate(make(100, {96, 5})).empty());
  CHECK(!validate(make(100, {-1, 5})).empty());
  CHECK(!validate(make(100, {10, 0})).empty());
  CHECK(!validate(make(100, {10, -3})).empty());
  CHECK(!validate(make(100, {100, 1})).empty());
  CHECK(!validate(make(100, {10, INT64_MAX})).empty());
  CHECK(!validate(make(0, {0, 1})).empty());
  CHECK(!validate(make(-1, {})).empty());
  CHECK(!compact_validate(100, nullptr, 1).empty());
  CHECK(!compact_validate(100, nullptr, -1).empty());
  CHECK(!compact_validate((int64_t)1 << 31, nullptr, 0).empty());
  CHECK(validate(make(100, {10, 5, 15, 5})).empty());  // touching ranges are fine
  // random valid calls
  std::mt19937_64 rng(9);
  for (int trial = 0; trial < 300; ++trial) {
    const int64_t rows = 1 + (int64_t)(rng() % (trial % 5 ? 60000 : 600000));
    const int64_t span = 1 + (int64_t)(rng() % (trial % 3 ? 40 : 4000));
    std::vector<int64_t> ranges;
    int64_t at = 0;
    for (;;) {
      const int64_t first = at + (int64_t)(rng() % span), count = 1 + (int64_t)(rng() % span);
      if (first >= rows || count > rows - first) break;
      ranges.push_back(first);
      ranges.push_back(count);
      at = first + count;
    }
    check_plan(make(rows, ranges), 1 + (int)(rng() % 3) * (int)(rng() % 50));
  }
  std::printf(g_fail ? "compact_plan_check: %d failures\n" : "compact_plan_check: ok\n", g_fail);
  return g_fail ? 1 : 0;
}
