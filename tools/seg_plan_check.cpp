// seg_plan_check.cpp — stand-alone host driver of the segmented search's work list (csrc/seg_plan.h): no
// device, no HIP.  Meant for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I rag-foundation_amd/csrc tools/seg_plan_check.cpp -o /tmp/seg_plan_check && /tmp/seg_plan_check
// It runs the validation over malformed inputs and the plan + device tables over random valid ones, in heap
// arrays of the exact length the arguments give (so any read past them is reported), and checks that every
// group's items tile its selected rows once and that every position maps into a validated range.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>

#include "seg_plan.h"

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
  int64_t rows, nq;
  int k, n_groups;
  std::unique_ptr<int64_t[]> gq, gr, ranges;  // exact lengths
};

static Call make(int64_t rows, int k, const std::vector<int64_t>& gq, const std::vector<int64_t>& gr,
                 const std::vector<int64_t>& ranges, int64_t nq) {
  Call c;
  c.rows = rows;
  c.nq = nq;
  c.k = k;
  c.n_groups = (int)gq.size() - 1;
  c.gq.reset(new int64_t[gq.size()]);
  c.gr.reset(new int64_t[gr.size()]);
  c.ranges.reset(new int64_t[ranges.size()]);
  std::copy(gq.begin(), gq.end(), c.gq.get());
  std::copy(gr.begin(), gr.end(), c.gr.get());
  std::copy(ranges.begin(), ranges.end(), c.ranges.get());
  return c;
}

static std::string validate(const Call& c) {
  return seg_validate(c.rows, c.nq, c.k, c.n_groups, c.gq.get(), c.gr.get(), c.ranges.get());
}

static void check_plan(const Call& c) {
  CHECK(validate(c).empty());
  std::vector<SegItem> items;
  const int lists = seg_plan(c.nq, c.n_groups, c.gq.get(), c.gr.get(), c.ranges.get(), items);
  CHECK(lists >= 1 && lists <= kSegLists);
  CHECK((int64_t)items.size() <= seg_max_items(c.nq));
  const int64_t n_ranges = c.gr[c.n_groups];
  std::unique_ptr<SegRangeDev[]> R(new SegRangeDev[n_ranges]);
  seg_ranges_dev(c.n_groups, c.gr.get(), c.ranges.get(), R.get());
  for (size_t i = 1; i < items.size(); ++i) CHECK(items[i - 1].n >= items[i].n);
  for (int g = 0; g < c.n_groups; ++g) {
    int64_t total = 0;
    for (int64_t i = c.gr[g]; i < c.gr[g + 1]; ++i) total += c.ranges[2 * i + 1];
    for (int64_t q0 = c.gq[g]; q0 < c.gq[g + 1]; q0 += kSegSlice) {
      std::vector<char> seen(total, 0);
      for (const SegItem& it : items) {
        if (it.group != g || it.q0 != q0) continue;
        const SegItemDev d = seg_item_dev(it);
        CHECK(d.nqt >= 1 && d.nqt <= kSegSlice && d.q0 + d.nqt <= c.gq[g + 1]);
        CHECK(d.list >= 0 && d.list < lists);
        CHECK(d.r_lo >= c.gr[g] && d.r_lo < d.r_hi && d.r_hi == c.gr[g + 1]);
        CHECK(R[d.r_lo].pos0 <= d.pos0 && d.pos0 < R[d.r_lo].pos1);  // the chunk starts inside range r_lo
        int ri = d.r_lo;
        for (int p = d.pos0; p < d.pos0 + d.n; ++p) {  // the kernel's walk
          while (p >= R[ri].pos1) ++ri;
          CHECK(ri < d.r_hi);
          const int64_t row = (int64_t)R[ri].row0 + (p - R[ri].pos0);
          CHECK(row >= c.ranges[2 * ri] && row < c.ranges[2 * ri] + c.ranges[2 * ri + 1] && row < c.rows);
          CHECK(p < total && !seen[p]);
          seen[p] = 1;
        }
      }
      for (int64_t p = 0; p < total; ++p) CHECK(seen[p]);
    }
  }
}

int main() {
  // hand-made: file-shaped ranges, a group without ranges, a group without queries
  check_plan(make(20011, 10, {0, 1, 9, 18, 58, 60, 60}, {0, 1, 4, 5, 9, 9, 10},
                  {0, 20011, 0, 7, 31, 2, 1000, 337, 5000, 1, 0, 7, 31, 2, 1000, 337, 15000, 5011, 3, 4}, 60));
  check_plan(make(100, 1, {0}, {0}, {}, 0));
  check_plan(make(0, 64, {0, 3}, {0, 0}, {}, 3));
  // malformed
  CHECK(!validate(make(100, 10, {0, 1}, {0, 2}, {50, 5, 10, 5}, 1)).empty());
  CHECK(!validate(make(100, 10, {0, 1}, {0, 2}, {10, 5, 14, 5}, 1)).empty());
  CHECK(!validate(make(100, 10, {0, 1}, {0, 1}, {96, 5}, 1)).empty());
  CHECK(!validate(make(100, 10, {0, 1}, {0, 1}, {-1, 5}, 1)).empty());
  CHECK(!validate(make(100, 10, {0, 1}, {0, 1}, {10, 0}, 1)).empty());
  CHECK(!validate(make(100, 10, {0, 1}, {0, 1}, {10, INT64_MAX}, 1)).empty());
  CHECK(!validate(make(100, 10, {0, 3, 2, 4}, {0, 1, 2, 3}, {0, 1, 2, 1, 4, 1}, 4)).empty());
  CHECK(!validate(make(100, 10, {0, 1, 2, 3}, {0, 2, 1, 3}, {0, 1, 2, 1, 4, 1}, 3)).empty());
  CHECK(!validate(make(100, 10, {0, 2, 4}, {0, 1, 2}, {0, 1, 2, 1}, 5)).empty());
  CHECK(!validate(make(100, 0, {0, 1}, {0, 1}, {0, 1}, 1)).empty());
  CHECK(!validate(make(100, 65, {0, 1}, {0, 1}, {0, 1}, 1)).empty());
  CHECK(!validate(make(100, 10, {0, kSegMaxNq + 1}, {0, 1}, {0, 1}, kSegMaxNq + 1)).empty());
  CHECK(!validate(make(100, 10, {0}, {0}, {}, 2)).empty());
  // random valid calls
  std::mt19937_64 rng(5);
  for (int trial = 0; trial < 300; ++trial) {
    const int64_t rows = 1 + (int64_t)(rng() % 60000);
    const int n_groups = 1 + (int)(rng() % 12);
    std::vector<int64_t> gq{0}, gr{0}, ranges;
    for (int g = 0; g < n_groups; ++g) {
      gq.push_back(gq.back() + (int64_t)(rng() % 20));
      int64_t at = 0;
      const int nr = (int)(rng() % 40);
      const int64_t span = 1 + (int64_t)(rng() % (trial % 3 ? 40 : 4000));
      for (int i = 0; i < nr; ++i) {
        const int64_t first = at + (int64_t)(rng() % span), count = 1 + (int64_t)(rng() % span);
        if (first >= rows || count > rows - first) break;
        ranges.push_back(first);
        ranges.push_back(count);
        at = first + count;
      }
      gr.push_back((int64_t)ranges.size() / 2);
    }
    check_plan(make(rows, 1 + (int)(rng() % 64), gq, gr, ranges, gq.back()));
  }
  std::printf(g_fail ? "seg_plan_check: %d failures\n" : "seg_plan_check: ok\n", g_fail);
  return g_fail ? 1 : 0;
}
