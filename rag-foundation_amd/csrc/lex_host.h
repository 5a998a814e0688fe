// lex_host.h — host-only: the lexical (BM25) index's bookkeeping (rfx_lex_*; kernels: k_lex.h, k_fuse.h).
// Plain C++ (no HIP): the library includes it, and so can a stand-alone host program (tools/lex_host_check.cpp:
// sanitizer runs of the append / tombstone / statistics / weight-table logic need no device).
//
// Path: the retrieval slice of ask_stream (gemini_rag.py:517-551) ranks by the dense embedding alone; the
// per-chunk hashed term features rfx_featurize already produces for the embedder are kept here as a CSR
// (one packed u32 per entry, bucket | tf << 16) with exact store statistics over the LIVE rows, so a keyword
// ranker (BM25) can run beside the dense search.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

namespace rfx {

constexpr int kLexMaxV = 65536;      // a bucket fits the packed entry's low 16 bits
constexpr int kLexMaxTf = 65535;     // tf is clamped here (int16 counts cannot reach it)
constexpr int kLexMaxNq = 1024;
constexpr int kLexMaxK = 64;
constexpr int kLexGroup = 8;         // questions per weight table

inline uint32_t lex_pack(int bucket, int tf) { return (uint32_t)bucket | ((uint32_t)tf << 16); }
inline int lex_bucket(uint32_t e) { return (int)(e & 0xffffu); }
inline int lex_tf(uint32_t e) { return (int)(e >> 16); }

// Returns "" when (indptr, bucket) is a CSR of n rows over V buckets: indptr[0] >= 0, monotone, buckets in [0, V).
template <class IP>
inline std::string lex_validate_csr(int V, const IP* indptr, const int32_t* bucket, const int16_t* count, int64_t n) {
  if (n < 0) return "n < 0";
  if (n == 0) return "";
  if (!indptr) return "null indptr";
  if (indptr[0] < 0) return "indptr[0] < 0";
  for (int64_t i = 0; i < n; ++i)
    if (indptr[i + 1] < indptr[i]) return "indptr not monotone (row " + std::to_string(i) + ")";
  const int64_t e0 = indptr[0], e1 = indptr[n];
  if (e1 > e0 && (!bucket || !count)) return "null bucket / count";
  for (int64_t e = e0; e < e1; ++e)
    if (bucket[e] < 0 || bucket[e] >= V) return "bucket " + std::to_string(bucket[e]) + " outside [0, V)";
  return "";
}

// One row's entries, packed: tf = |count| (the hash sign is dropped), zero counts dropped, sorted by bucket,
// a repeated bucket merged (tf summed), tf clamped at kLexMaxTf.  Appends to `out`; returns len_r = sum of tf.
inline int64_t lex_pack_row(const int32_t* bucket, const int16_t* count, int64_t e0, int64_t e1,
                            std::vector<uint32_t>& out) {
  const size_t first = out.size();
  bool sorted = true;
  int prev = -1;
  for (int64_t e = e0; e < e1; ++e) {
    const int c = count[e] < 0 ? -(int)count[e] : (int)count[e];
    if (c == 0) continue;
    if (bucket[e] <= prev) sorted = false;
    prev = bucket[e];
    out.push_back(lex_pack(bucket[e], std::min(c, kLexMaxTf)));
  }
  if (!sorted) {
    std::sort(out.begin() + (ptrdiff_t)first, out.end(),
              [](uint32_t a, uint32_t b) { return lex_bucket(a) < lex_bucket(b); });
    size_t w = first;
    for (size_t i = first; i < out.size(); ++i) {
      if (w > first && lex_bucket(out[w - 1]) == lex_bucket(out[i]))
        out[w - 1] = lex_pack(lex_bucket(out[i]), std::min(lex_tf(out[w - 1]) + lex_tf(out[i]), kLexMaxTf));
      else
        out[w++] = out[i];
    }
    out.resize(w);
  }
  int64_t len = 0;
  for (size_t i = first; i < out.size(); ++i) len += lex_tf(out[i]);
  return len;
}

// The host mirror of the index: every row's packed entries (a tombstone must know the row's buckets) and the
// statistics over live rows, exact integers.
struct LexHost {
  int V = 0;
  int64_t rows = 0, live = 0, nnz = 0, total_len = 0;  // total_len: over live rows
  std::vector<int64_t> indptr{0};                      // [rows + 1]
  std::vector<uint32_t> entries;                       // [nnz]
  std::vector<int32_t> len;                            // [rows], -1 = dead
  std::vector<int64_t> df;                             // [V], live rows holding the bucket

  explicit LexHost(int v = 0) : V(v), df((size_t)v, 0) {}

  // Appends n VALID rows (lex_validate_csr passed).  The new rows are [rows_before, rows); their packed
  // entries entries[indptr[rows_before] ..).
  template <class IP>
  void append(const IP* ip, const int32_t* bucket, const int16_t* count, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
      const size_t first = entries.size();
      const int64_t l = lex_pack_row(bucket, count, (int64_t)ip[i], (int64_t)ip[i + 1], entries);
      for (size_t e = first; e < entries.size(); ++e) ++df[(size_t)lex_bucket(entries[e])];
      len.push_back((int32_t)std::min<int64_t>(l, 0x7fffffff));
      indptr.push_back((int64_t)entries.size());
      total_len += len.back();
      ++rows;
      ++live;
    }
    nnz = (int64_t)entries.size();
  }

  // "" when every row is in [0, rows)
  std::string validate_rows(const int64_t* r, int64_t n) const {
    if (n < 0) return "n < 0";
    if (n > 0 && !r) return "null rows";
    for (int64_t i = 0; i < n; ++i)
      if (r[i] < 0 || r[i] >= rows) return "row " + std::to_string(r[i]) + " outside [0, rows)";
    return "";
  }

  // Tombstones VALID rows: a live row leaves the statistics (a dead one is skipped).  Returns the rows that died.
  int64_t tombstone(const int64_t* r, int64_t n) {
    int64_t died = 0;
    for (int64_t i = 0; i < n; ++i) {
      const size_t row = (size_t)r[i];
      if (len[row] < 0) continue;
      for (int64_t e = indptr[row]; e < indptr[row + 1]; ++e) --df[(size_t)lex_bucket(entries[(size_t)e])];
      total_len -= len[row];
      len[row] = -1;
      --live;
      ++died;
    }
    return died;
  }

  double avgdl() const { return (double)total_len / (double)live; }
  // idf_t = log(1 + ((N - df) + 0.5) / (df + 0.5)), f64, each operation rounded on its own
  double idf(int t) const {
    const double num = (double)(live - df[(size_t)t]) + 0.5, den = (double)df[(size_t)t] + 0.5;
    const double ratio = num / den;
    return log(1.0 + ratio);
  }
};

struct LexQueryEntry {  // 8 B, the device's sparse question entry
  uint32_t bucket;
  float w;
};

// The weight tables of VALID questions: per question its distinct buckets with w = fl32(idf * qtf), qtf =
// |count| (zero counts dropped, a repeated bucket merged).  off: [nq + 1] entry offsets.
template <class IP>
inline void lex_query_weights(const LexHost& L, const IP* q_indptr, const int32_t* q_bucket, const int16_t* q_count,
                              int64_t nq, std::vector<int32_t>& off, std::vector<LexQueryEntry>& ent) {
  off.assign(1, 0);
  ent.clear();
  std::vector<uint32_t> row;
  for (int64_t q = 0; q < nq; ++q) {
    row.clear();
    lex_pack_row(q_bucket, q_count, (int64_t)q_indptr[q], (int64_t)q_indptr[q + 1], row);
    for (uint32_t e : row) {
      const double w = L.idf(lex_bucket(e)) * (double)lex_tf(e);
      ent.push_back(LexQueryEntry{(uint32_t)lex_bucket(e), (float)w});
    }
    off.push_back((int32_t)ent.size());
  }
}

// "" when the arguments of a search are acceptable (the question CSR is checked with lex_validate_csr)
inline std::string lex_validate_search(int64_t nq, int k, float k1, float b) {
  if (nq < 1 || nq > kLexMaxNq) return "nq=" + std::to_string(nq) + " out of [1, 1024]";
  if (k < 1 || k > kLexMaxK) return "k=" + std::to_string(k) + " out of [1, 64]";
  if (!(k1 >= 0.0f) || isinf(k1)) return "k1 must be a finite number >= 0";
  if (!(b >= 0.0f && b <= 1.0f)) return "b outside [0, 1]";
  return "";
}

// "" when the arguments of a fusion are acceptable; alpha / n_dense / n_lex may be null (0.5, the list maxima)
inline std::string lex_validate_fuse(int n_dense_max, int n_lex_max, int64_t nq, int k, const float* alpha,
                                     const int32_t* n_dense, const int32_t* n_lex, int rrf_c) {
  if (nq < 1 || nq > kLexMaxNq) return "nq=" + std::to_string(nq) + " out of [1, 1024]";
  if (k < 1 || k > kLexMaxK) return "k=" + std::to_string(k) + " out of [1, 64]";
  if (n_dense_max < 1 || n_dense_max > 64) return "n_dense_max=" + std::to_string(n_dense_max) + " out of [1, 64]";
  if (n_lex_max < 1 || n_lex_max > 64) return "n_lex_max=" + std::to_string(n_lex_max) + " out of [1, 64]";
  if (k > n_dense_max + n_lex_max) return "k > n_dense_max + n_lex_max";
  if (rrf_c < 1) return "rrf_c < 1";
  for (int64_t q = 0; q < nq; ++q) {
    const std::string at = " (question " + std::to_string(q) + ")";
    if (alpha && !(alpha[q] >= 0.0f && alpha[q] <= 1.0f)) return "alpha outside [0, 1]" + at;  // (a NaN fails both)
    if (n_dense && (n_dense[q] < 1 || n_dense[q] > n_dense_max)) return "n_dense outside [1, n_dense_max]" + at;
    if (n_lex && (n_lex[q] < 1 || n_lex[q] > n_lex_max)) return "n_lex outside [1, n_lex_max]" + at;
  }
  return "";
}

// growth by doubling: the capacity that holds `need` elements, from `cap`
inline int64_t lex_grow(int64_t cap, int64_t need, int64_t least) {
  int64_t c = std::max(cap, least);
  while (c < need) c *= 2;
  return c;
}

}  // namespace rfx
