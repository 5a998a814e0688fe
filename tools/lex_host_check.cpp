// lex_host_check.cpp — stand-alone host driver of the lexical index's bookkeeping (csrc/lex_host.h): no
// HIP, no device.  Build it with the host compiler and sanitizers and run it:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I rag-foundation_amd/csrc tools/lex_host_check.cpp -o /tmp/lex_host_check && /tmp/lex_host_check
// It covers append (packing, |count|, zero counts, unsorted and repeated buckets), tombstone, the statistics
// against a fresh build over the live rows, the idf / weight tables, and every refused argument.
#include <cmath>
#include <cstdio>
#include <limits>

#include "lex_host.h"

static int g_fail = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      ++g_fail;                                                       \
    }                                                                 \
  } while (0)

static uint64_t sm64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

struct Csr {
  std::vector<int32_t> ip{0}, bk;
  std::vector<int16_t> ct;
};

// n rows of 0..39 sorted distinct buckets over V, counts in -9..9 (zeros included)
static Csr gen(uint64_t seed, int n, int V) {
  Csr c;
  for (int r = 0; r < n; ++r) {
    const int m = (int)(sm64(seed + (uint64_t)r) % 40);
    std::vector<int> b;
    for (int j = 0; j < m; ++j) b.push_back((int)(sm64(seed * 31 + (uint64_t)r * 64 + (uint64_t)j) % (uint64_t)V));
    std::sort(b.begin(), b.end());
    b.erase(std::unique(b.begin(), b.end()), b.end());
    for (size_t j = 0; j < b.size(); ++j) {
      c.bk.push_back(b[j]);
      c.ct.push_back((int16_t)((int)(sm64(seed + 977 * (uint64_t)r + j) % 19) - 9));
    }
    c.ip.push_back((int32_t)c.bk.size());
  }
  return c;
}

static Csr rows_of(const Csr& c, const std::vector<int>& rows) {
  Csr o;
  for (int r : rows) {
    for (int e = c.ip[(size_t)r]; e < c.ip[(size_t)r + 1]; ++e) o.bk.push_back(c.bk[(size_t)e]), o.ct.push_back(c.ct[(size_t)e]);
    o.ip.push_back((int32_t)o.bk.size());
  }
  return o;
}

int main() {
  using namespace rfx;
  const int V = 256;
  // ---- packing ----
  {
    const int32_t bk[] = {7, 3, 7, 200, 5};
    const int16_t ct[] = {-2, 4, 3, 0, -256};
    std::vector<uint32_t> out;
    const int64_t len = lex_pack_row(bk, ct, 0, 5, out);  // unsorted, repeated 7, a zero count
    CHECK(out.size() == 3);
    CHECK(out[0] == lex_pack(3, 4) && out[1] == lex_pack(5, 256) && out[2] == lex_pack(7, 5));
    CHECK(len == 265);
    CHECK(lex_bucket(lex_pack(65535, 65535)) == 65535 && lex_tf(lex_pack(65535, 65535)) == 65535);
  }
  // ---- append / tombstone / statistics == a fresh build over the live rows ----
  const Csr all = gen(11, 300, V);
  LexHost L(V);
  CHECK(lex_validate_csr(V, all.ip.data(), all.bk.data(), all.ct.data(), 300).empty());
  L.append(all.ip.data(), all.bk.data(), all.ct.data(), 100);
  L.append(all.ip.data() + 100, all.bk.data(), all.ct.data(), 200);  // indptr that does not start at 0
  CHECK(L.rows == 300 && L.live == 300 && (int64_t)L.indptr.size() == 301 && L.nnz == (int64_t)L.entries.size());
  std::vector<int64_t> dead;
  std::vector<int> live;
  for (int r = 0; r < 300; ++r) (sm64(5 + (uint64_t)r) % 3 == 0 ? (void)dead.push_back(r) : (void)live.push_back(r));
  CHECK(L.validate_rows(dead.data(), (int64_t)dead.size()).empty());
  CHECK(L.tombstone(dead.data(), (int64_t)dead.size()) == (int64_t)dead.size());
  CHECK(L.tombstone(dead.data(), (int64_t)dead.size()) == 0);  // twice: nothing more leaves
  const Csr lv = rows_of(all, live);
  LexHost F(V);
  F.append(lv.ip.data(), lv.bk.data(), lv.ct.data(), (int64_t)live.size());
  CHECK(F.live == L.live && F.total_len == L.total_len && F.df == L.df);
  CHECK(L.rows == 300 && L.live == (int64_t)live.size());
  for (int64_t r : dead) CHECK(L.len[(size_t)r] == -1);
  for (int t = 0; t < V; ++t) CHECK(L.idf(t) == F.idf(t) && L.idf(t) > 0.0);
  CHECK(L.avgdl() == F.avgdl());
  // every row's entries are sorted, tf >= 1, and len is their sum
  for (int r = 0; r < 300; ++r) {
    int64_t s = 0;
    for (int64_t e = L.indptr[(size_t)r]; e < L.indptr[(size_t)r + 1]; ++e) {
      CHECK(lex_tf(L.entries[(size_t)e]) >= 1);
      if (e > L.indptr[(size_t)r]) CHECK(lex_bucket(L.entries[(size_t)e - 1]) < lex_bucket(L.entries[(size_t)e]));
      s += lex_tf(L.entries[(size_t)e]);
    }
    CHECK(L.len[(size_t)r] == -1 || L.len[(size_t)r] == s);
  }
  // ---- weight tables ----
  {
    const int32_t qip[] = {0, 3, 3, 5};
    const int32_t qbk[] = {9, 4, 9, 100, 101};
    const int16_t qct[] = {1, -1, 2, 0, 3};  // question 0 repeats bucket 9 (qtf 3); question 1 is empty
    std::vector<int32_t> off;
    std::vector<LexQueryEntry> ent;
    CHECK(lex_validate_csr(V, qip, qbk, qct, 3).empty());
    lex_query_weights(L, qip, qbk, qct, 3, off, ent);
    CHECK(off.size() == 4 && off[0] == 0 && off[1] == 2 && off[2] == 2 && off[3] == 3);
    CHECK(ent[0].bucket == 4 && ent[0].w == (float)(L.idf(4) * 1.0));
    CHECK(ent[1].bucket == 9 && ent[1].w == (float)(L.idf(9) * 3.0));
    CHECK(ent[2].bucket == 101 && ent[2].w == (float)(L.idf(101) * 3.0));
  }
  // ---- refused arguments ----
  {
    const int32_t ip_bad[] = {0, 2, 1};
    const int32_t bk[] = {1, 2};
    const int16_t ct[] = {1, 1};
    CHECK(!lex_validate_csr(V, ip_bad, bk, ct, 2).empty());  // non-monotone
    const int32_t ip_neg[] = {-1, 1};
    CHECK(!lex_validate_csr(V, ip_neg, bk, ct, 1).empty());
    const int32_t ip[] = {0, 2};
    const int32_t bk_hi[] = {1, V};
    const int32_t bk_lo[] = {-1, 2};
    CHECK(!lex_validate_csr(V, ip, bk_hi, ct, 1).empty());  // bucket >= V
    CHECK(!lex_validate_csr(V, ip, bk_lo, ct, 1).empty());
    CHECK(!lex_validate_csr(V, ip, (const int32_t*)nullptr, ct, 1).empty());
    CHECK(!lex_validate_csr(V, ip, bk, ct, -1).empty());
    CHECK(lex_validate_csr(V, ip, bk, ct, 1).empty());
    const int64_t out_rows[] = {0, 300};
    const int64_t neg_rows[] = {-1};
    CHECK(!L.validate_rows(out_rows, 2).empty() && !L.validate_rows(neg_rows, 1).empty());
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    CHECK(lex_validate_search(1, 1, 1.2f, 0.75f).empty() && lex_validate_search(1024, 64, 0.0f, 1.0f).empty());
    CHECK(!lex_validate_search(0, 10, 1.2f, 0.75f).empty() && !lex_validate_search(1025, 10, 1.2f, 0.75f).empty());
    CHECK(!lex_validate_search(1, 0, 1.2f, 0.75f).empty() && !lex_validate_search(1, 65, 1.2f, 0.75f).empty());
    CHECK(!lex_validate_search(1, 10, -0.1f, 0.75f).empty() && !lex_validate_search(1, 10, nan, 0.75f).empty());
    CHECK(!lex_validate_search(1, 10, inf, 0.75f).empty());
    CHECK(!lex_validate_search(1, 10, 1.2f, -0.1f).empty() && !lex_validate_search(1, 10, 1.2f, 1.1f).empty());
    CHECK(!lex_validate_search(1, 10, 1.2f, nan).empty());
    const float a_ok[] = {0.0f, 1.0f}, a_hi[] = {0.5f, 1.5f}, a_nan[] = {nan, 0.5f};
    const int32_t n_ok[] = {1, 10}, n_zero[] = {0, 10}, n_big[] = {1, 11};
    CHECK(lex_validate_fuse(10, 10, 2, 10, a_ok, n_ok, n_ok, 60).empty());
    CHECK(lex_validate_fuse(64, 64, 1, 64, nullptr, nullptr, nullptr, 1).empty());
    CHECK(!lex_validate_fuse(10, 10, 2, 10, a_hi, n_ok, n_ok, 60).empty());
    CHECK(!lex_validate_fuse(10, 10, 2, 10, a_nan, n_ok, n_ok, 60).empty());
    CHECK(!lex_validate_fuse(10, 10, 2, 10, a_ok, n_zero, n_ok, 60).empty());
    CHECK(!lex_validate_fuse(10, 10, 2, 10, a_ok, n_ok, n_big, 60).empty());
    CHECK(!lex_validate_fuse(10, 10, 2, 10, a_ok, n_ok, n_ok, 0).empty());
    CHECK(!lex_validate_fuse(10, 10, 2, 21, a_ok, n_ok, n_ok, 60).empty());  // k > n_dense_max + n_lex_max
    CHECK(!lex_validate_fuse(0, 10, 2, 5, a_ok, nullptr, n_ok, 60).empty());
    CHECK(!lex_validate_fuse(10, 65, 2, 5, a_ok, n_ok, nullptr, 60).empty());
    CHECK(!lex_validate_fuse(10, 10, 0, 5, nullptr, nullptr, nullptr, 60).empty());
    CHECK(!lex_validate_fuse(10, 10, 1025, 5, nullptr, nullptr, nullptr, 60).empty());
    CHECK(!lex_validate_fuse(10, 10, 2, 0, a_ok, n_ok, n_ok, 60).empty());
    CHECK(!lex_validate_fuse(40, 40, 2, 65, a_ok, n_ok, n_ok, 60).empty());
  }
  CHECK(lex_grow(0, 1, 4096) == 4096 && lex_grow(4096, 4097, 4096) == 8192 && lex_grow(8192, 40000, 4096) == 65536);
  std::printf(g_fail ? "lex_host_check: %d failures\n" : "lex_host_check: ok\n", g_fail);
  return g_fail ? 1 : 0;
}
