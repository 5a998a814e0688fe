// lex_api.hip — C ABI of the lexical (BM25) index and the rank fusion (include/rfx.h, "lexical index").
//
// One handle owns, on one device: the CSR of every row's hashed term features (indptr, packed entries, len) and,
// on the host, its mirror with the exact statistics over live rows (lex_host.h).  Kernels: k_lex.hip, k_fuse.hip;
// rules: DESIGN §4.14, restated in numpy by tests/lex_ref.py.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "k_fuse.h"
#include "k_lex.h"
#include "rfx_kernels.h"

namespace {

using rfx::api_fail;

#define LEX_HIP(call)                                                                             \
  do {                                                                                            \
    hipError_t e_ = (call);                                                                       \
    if (e_ != hipSuccess) return api_fail(RFX_EDEVICE, "%s: %s", #call, hipGetErrorString(e_));   \
  } while (0)

struct Lex {
  int device = 0;
  std::mutex mu;
  rfx::LexHost host;
  int64_t cap_rows = 0, cap_nnz = 0;
  int64_t* indptr = nullptr;   // [cap_rows + 1]
  uint32_t* entries = nullptr;  // [cap_nnz]
  int32_t* len = nullptr;       // [cap_rows]
  void* stage = nullptr;        // pinned staging (appends, question tables, fusion tables)
  size_t stage_bytes = 0;
  hipEvent_t stage_ev = nullptr;  // the last stream-ordered copy out of the staging buffer
  void* fuse_tab = nullptr;       // device: the fusion's per-question tables, 3 x [kLexMaxNq]
  explicit Lex(int V) : host(V) {}
  ~Lex() {
    for (void* p : {(void*)indptr, (void*)entries, (void*)len, fuse_tab})
      if (p) (void)hipFree(p);
    if (stage) (void)hipHostFree(stage);
    if (stage_ev) (void)hipEventDestroy(stage_ev);
  }
};

std::mutex g_mu;
std::map<uint64_t, std::shared_ptr<Lex>> g_lex;
std::atomic<uint64_t> g_next{1};

std::shared_ptr<Lex> get(rfx_lex_t h) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_lex.find(h);
  return it == g_lex.end() ? nullptr : it->second;
}

size_t al256(size_t x) { return (x + 255) / 256 * 256; }

// the staging buffer, free of any copy still in flight, at least `need` bytes
int stage_acquire(Lex& lx, size_t need) {
  if (!lx.stage_ev) LEX_HIP(hipEventCreateWithFlags(&lx.stage_ev, hipEventDisableTiming));
  else LEX_HIP(hipEventSynchronize(lx.stage_ev));
  if (lx.stage_bytes < need) {
    if (lx.stage) LEX_HIP(hipHostFree(lx.stage));
    lx.stage = nullptr;
    lx.stage_bytes = 0;
    const size_t want = std::max(need * 2, (size_t)1 << 16);
    if (hipHostMalloc(&lx.stage, want, hipHostMallocDefault) != hipSuccess)
      return api_fail(RFX_ENOMEM, "hipHostMalloc(%zu) failed (lexical staging)", want);
    lx.stage_bytes = want;
  }
  return RFX_OK;
}

// host -> device through the pinned staging buffer, in pieces; synchronous
int upload(Lex& lx, void* dst, const void* src, size_t bytes) {
  constexpr size_t kPiece = (size_t)8 << 20;
  for (size_t o = 0; o < bytes; o += kPiece) {
    const size_t n = std::min(kPiece, bytes - o);
    if (const int rc = stage_acquire(lx, n)) return rc;
    std::memcpy(lx.stage, (const uint8_t*)src + o, n);
    LEX_HIP(hipMemcpyAsync((uint8_t*)dst + o, lx.stage, n, hipMemcpyHostToDevice, nullptr));
    LEX_HIP(hipEventRecord(lx.stage_ev, nullptr));
  }
  LEX_HIP(hipStreamSynchronize(nullptr));
  return RFX_OK;
}

template <class T>
int regrow(T*& p, int64_t used, int64_t new_n) {
  T* q = nullptr;
  if (hipMalloc(&q, (size_t)new_n * sizeof(T)) != hipSuccess)
    return api_fail(RFX_ENOMEM, "hipMalloc(%zu) failed (lexical index)", (size_t)new_n * sizeof(T));
  if (p && used > 0) {
    const hipError_t e = hipMemcpy(q, p, (size_t)used * sizeof(T), hipMemcpyDeviceToDevice);
    if (e != hipSuccess) {
      (void)hipFree(q);
      return api_fail(RFX_EDEVICE, "hipMemcpy: %s", hipGetErrorString(e));
    }
  }
  LEX_HIP(hipDeviceSynchronize());  // searches enqueued on any stream are done with the old allocation
  if (p) LEX_HIP(hipFree(p));
  p = q;
  return RFX_OK;
}

struct LexWs {  // workspace layout of a search
  rfx::LexPlan p;
  size_t off_off, ent_off, w_off, cs_off, cr_off, total;
};
LexWs lex_ws(const Lex& lx, int64_t nq, int k, int64_t q_nnz_cap) {
  LexWs w{};
  w.p = rfx::lex_plan(std::max<int64_t>(lx.host.rows, 1), lx.host.V, nq, k);
  size_t o = 0;
  w.off_off = o, o += al256((size_t)(nq + 1) * 4);
  w.ent_off = o, o += al256((size_t)q_nnz_cap * sizeof(rfx::LexQueryEntry));
  w.w_off = o, o += al256((size_t)w.p.groups * lx.host.V * w.p.nqt * 4);
  const size_t cand = (size_t)nq * w.p.blocks * w.p.k_slot;
  w.cs_off = o, o += al256(cand * 4);
  w.cr_off = o, o += al256(cand * 4);
  w.total = o;
  return w;
}
// a question holds at most V distinct buckets; the workspace covers min(V, 4096) per question (a chunk's
// featurisation has far fewer), a longer batch is refused
int64_t q_nnz_cap(const Lex& lx, int64_t nq) { return nq * std::min(lx.host.V, 4096); }

}  // namespace

extern "C" {

int rfx_lex_create(int V, int device, rfx_lex_t* out) {
  if (!out) return api_fail(RFX_EINVAL, "null output");
  if (V < 1 || V > rfx::kLexMaxV) return api_fail(RFX_EINVAL, "V=%d out of [1, %d]", V, rfx::kLexMaxV);
  int n = 0;
  LEX_HIP(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return api_fail(RFX_EINVAL, "device %d out of [0, %d)", device, n);
  auto lx = std::make_shared<Lex>(V);
  lx->device = device;
  const uint64_t h = g_next++;
  std::lock_guard<std::mutex> lk(g_mu);
  g_lex[h] = lx;
  *out = h;
  return RFX_OK;
}

int rfx_lex_destroy(rfx_lex_t h) {
  std::shared_ptr<Lex> lx;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_lex.find(h);
    if (it == g_lex.end()) return api_fail(RFX_EINVAL, "unknown lexical handle");
    lx = it->second;
    g_lex.erase(it);
  }
  std::lock_guard<std::mutex> lk(lx->mu);
  (void)hipSetDevice(lx->device);
  (void)hipDeviceSynchronize();  // nothing enqueued may still read the index
  return RFX_OK;
}

int rfx_lex_add(rfx_lex_t h, const int32_t* indptr_h, const int32_t* bucket_h, const int16_t* count_h, int64_t n) {
  auto lx = get(h);
  if (!lx) return api_fail(RFX_EINVAL, "unknown lexical handle");
  std::lock_guard<std::mutex> lk(lx->mu);
  rfx::LexHost& H = lx->host;
  const std::string err = rfx::lex_validate_csr(H.V, indptr_h, bucket_h, count_h, n);
  if (!err.empty()) return api_fail(RFX_EINVAL, "lex add: %s", err.c_str());
  if (n == 0) return RFX_OK;
  if (H.rows + n >= 0x7fffffffll) return api_fail(RFX_EINVAL, "lex add: more than 2^31 - 2 rows");
  LEX_HIP(hipSetDevice(lx->device));
  const int64_t rows0 = H.rows, nnz0 = H.nnz;
  H.append(indptr_h, bucket_h, count_h, n);
  int rc = RFX_OK;
  if (H.rows > lx->cap_rows) {
    const int64_t cap = rfx::lex_grow(lx->cap_rows, H.rows, 4096);
    // (indptr holds one more element than there are rows)
    if (!(rc = regrow(lx->indptr, lx->cap_rows ? rows0 + 1 : 0, cap + 1)) && !(rc = regrow(lx->len, rows0, cap)))
      lx->cap_rows = cap;
  }
  if (!rc && H.nnz > lx->cap_nnz) {
    const int64_t cap = rfx::lex_grow(lx->cap_nnz, H.nnz, 1 << 16);
    if (!(rc = regrow(lx->entries, nnz0, cap))) lx->cap_nnz = cap;
  }
  if (!rc) rc = upload(*lx, lx->indptr + rows0, H.indptr.data() + rows0, (size_t)(n + 1) * 8);
  if (!rc) rc = upload(*lx, lx->len + rows0, H.len.data() + rows0, (size_t)n * 4);
  if (!rc && H.nnz > nnz0) rc = upload(*lx, lx->entries + nnz0, H.entries.data() + nnz0, (size_t)(H.nnz - nnz0) * 4);
  if (rc) {  // the device does not hold the rows: take them out of the mirror again
    std::vector<int64_t> back((size_t)n);
    for (int64_t i = 0; i < n; ++i) back[(size_t)i] = rows0 + i;
    H.tombstone(back.data(), n);
    H.rows = rows0, H.nnz = nnz0;
    H.indptr.resize((size_t)rows0 + 1), H.len.resize((size_t)rows0), H.entries.resize((size_t)nnz0);
  }
  return rc;
}

int rfx_lex_tombstone(rfx_lex_t h, const int64_t* rows_h, int64_t n) {
  auto lx = get(h);
  if (!lx) return api_fail(RFX_EINVAL, "unknown lexical handle");
  std::lock_guard<std::mutex> lk(lx->mu);
  const std::string err = lx->host.validate_rows(rows_h, n);
  if (!err.empty()) return api_fail(RFX_EINVAL, "lex tombstone: %s", err.c_str());
  if (n == 0) return RFX_OK;
  LEX_HIP(hipSetDevice(lx->device));
  lx->host.tombstone(rows_h, n);
  int64_t* rows_d = nullptr;
  if (hipMalloc(&rows_d, (size_t)n * 8) != hipSuccess) return api_fail(RFX_ENOMEM, "hipMalloc failed (tombstone rows)");
  int rc = upload(*lx, rows_d, rows_h, (size_t)n * 8);
  if (!rc) {
    rfx::launch_lex_set_dead(lx->len, rows_d, n, nullptr);
    const hipError_t e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) rc = api_fail(RFX_EDEVICE, "lex tombstone: %s", hipGetErrorString(e));
  }
  (void)hipFree(rows_d);
  return rc;
}

int rfx_lex_info(rfx_lex_t h, int64_t* rows, int64_t* live, int64_t* nnz, int64_t* total_len) {
  auto lx = get(h);
  if (!lx) return api_fail(RFX_EINVAL, "unknown lexical handle");
  std::lock_guard<std::mutex> lk(lx->mu);
  if (rows) *rows = lx->host.rows;
  if (live) *live = lx->host.live;
  if (nnz) *nnz = lx->host.nnz;
  if (total_len) *total_len = lx->host.total_len;
  return RFX_OK;
}

int rfx_lex_df(rfx_lex_t h, int64_t* out) {
  auto lx = get(h);
  if (!lx) return api_fail(RFX_EINVAL, "unknown lexical handle");
  if (!out) return api_fail(RFX_EINVAL, "null output");
  std::lock_guard<std::mutex> lk(lx->mu);
  std::memcpy(out, lx->host.df.data(), (size_t)lx->host.V * 8);
  return RFX_OK;
}

int rfx_lex_search_workspace_bytes(rfx_lex_t h, int64_t nq, int k, size_t* out_bytes) {
  auto lx = get(h);
  if (!lx) return api_fail(RFX_EINVAL, "unknown lexical handle");
  if (!out_bytes) return api_fail(RFX_EINVAL, "null output");
  const std::string err = rfx::lex_validate_search(nq, k, 1.2f, 0.75f);
  if (!err.empty()) return api_fail(RFX_EINVAL, "lex search: %s", err.c_str());
  std::lock_guard<std::mutex> lk(lx->mu);
  *out_bytes = lex_ws(*lx, nq, k, q_nnz_cap(*lx, nq)).total;
  return RFX_OK;
}

int rfx_lex_search(rfx_lex_t h, const int32_t* q_indptr_h, const int32_t* q_bucket_h, const int16_t* q_count_h,
                   int64_t nq, int k, float k1, float b, const uint32_t* mask_d, int64_t mask_words, float* scores_d,
                   int64_t* rows_d, void* ws, size_t ws_bytes, void* stream) {
  auto lx = get(h);
  if (!lx) return api_fail(RFX_EINVAL, "unknown lexical handle");
  std::string err = rfx::lex_validate_search(nq, k, k1, b);
  if (!err.empty()) return api_fail(RFX_EINVAL, "lex search: %s", err.c_str());
  std::lock_guard<std::mutex> lk(lx->mu);
  const rfx::LexHost& H = lx->host;
  err = rfx::lex_validate_csr(H.V, q_indptr_h, q_bucket_h, q_count_h, nq);
  if (!err.empty()) return api_fail(RFX_EINVAL, "lex search: question %s", err.c_str());
  if (!scores_d || !rows_d) return api_fail(RFX_EINVAL, "lex search: null outputs");
  if (mask_d && mask_words < (H.rows + 31) / 32)
    return api_fail(RFX_EINVAL, "row mask has %lld words, the index needs %lld", (long long)mask_words,
                    (long long)((H.rows + 31) / 32));
  const int64_t cap = q_nnz_cap(*lx, nq);
  const LexWs W = lex_ws(*lx, nq, k, cap);
  if (!ws || ws_bytes < W.total) return api_fail(RFX_EINVAL, "workspace too small (%zu < %zu)", ws_bytes, W.total);
  std::vector<int32_t> off;
  std::vector<rfx::LexQueryEntry> ent;
  rfx::lex_query_weights(H, q_indptr_h, q_bucket_h, q_count_h, nq, off, ent);
  if ((int64_t)ent.size() > cap)
    return api_fail(RFX_EINVAL, "lex search: %zu question entries, the workspace holds %lld", ent.size(), (long long)cap);
  LEX_HIP(hipSetDevice(lx->device));
  hipStream_t st = (hipStream_t)stream;
  uint8_t* w8 = (uint8_t*)ws;
  float* cs = (float*)(w8 + W.cs_off);
  int* cr = (int*)(w8 + W.cr_off);
  if (H.rows == 0 || H.live == 0) {
    // nothing can rank: one empty list per question through the same merge
    const size_t n = (size_t)nq * W.p.k_slot;
    if (const int rc = stage_acquire(*lx, 2 * n * 4)) return rc;
    uint32_t* s32 = (uint32_t*)lx->stage;
    for (size_t i = 0; i < n; ++i) s32[i] = 0xff800000u, s32[n + i] = (uint32_t)0x7fffffff;
    LEX_HIP(hipMemcpyAsync(cs, s32, n * 4, hipMemcpyHostToDevice, st));
    LEX_HIP(hipMemcpyAsync(cr, s32 + n, n * 4, hipMemcpyHostToDevice, st));
    LEX_HIP(hipEventRecord(lx->stage_ev, st));
    if (rfx::launch_topk_merge_lists(cs, cr, 0, nq, W.p.k_slot, W.p.k_slot, k, 0, scores_d, rows_d, nullptr, st, true) != 0)
      return api_fail(RFX_EUNSUPPORTED, "lex search: merge k=%d unsupported", k);
    LEX_HIP(hipGetLastError());
    return RFX_OK;
  }
  {
    // the question tables through the pinned staging buffer: the caller's arrays may die on return
    const size_t need = W.ent_off + ent.size() * sizeof(rfx::LexQueryEntry);
    if (const int rc = stage_acquire(*lx, need)) return rc;
    uint8_t* s8 = (uint8_t*)lx->stage;
    std::memcpy(s8 + W.off_off, off.data(), off.size() * 4);
    if (!ent.empty()) std::memcpy(s8 + W.ent_off, ent.data(), ent.size() * sizeof(rfx::LexQueryEntry));
    LEX_HIP(hipMemcpyAsync(w8, s8, need, hipMemcpyHostToDevice, st));  // one copy: both tables and the gap
    LEX_HIP(hipEventRecord(lx->stage_ev, st));
  }
  rfx::launch_lex_weights(W.p, H.V, (const int32_t*)(w8 + W.off_off), (const rfx::LexQueryEntry*)(w8 + W.ent_off), nq,
                          (float*)(w8 + W.w_off), st);
  if (rfx::launch_lex_scan(W.p, H.V, lx->indptr, lx->entries, lx->len, H.rows, (const float*)(w8 + W.w_off), nq,
                           (double)k1, (double)b, H.avgdl(), mask_d, cs, cr, st) != 0)
    return api_fail(RFX_EUNSUPPORTED, "lex scan launch rejected");
  if (rfx::launch_topk_merge_lists(cs, cr, 0, nq, (int64_t)W.p.blocks * W.p.k_slot, W.p.k_slot, k, 0, scores_d, rows_d,
                                   nullptr, st, true) != 0)
    return api_fail(RFX_EUNSUPPORTED, "lex search: merge k=%d unsupported", k);
  LEX_HIP(hipGetLastError());
  return RFX_OK;
}

int rfx_lex_fuse(rfx_lex_t h, const int64_t* dense_rows_d, int n_dense_max, const int64_t* lex_rows_d, int n_lex_max,
                 int64_t nq, int k, const float* alpha_h, const int32_t* n_dense_h, const int32_t* n_lex_h, int rrf_c,
                 float* out_scores_d, int64_t* out_rows_d, int32_t* out_ranks_d, void* stream) {
  auto lx = get(h);
  if (!lx) return api_fail(RFX_EINVAL, "unknown lexical handle");
  const std::string err = rfx::lex_validate_fuse(n_dense_max, n_lex_max, nq, k, alpha_h, n_dense_h, n_lex_h, rrf_c);
  if (!err.empty()) return api_fail(RFX_EINVAL, "lex fuse: %s", err.c_str());
  if (!dense_rows_d || !lex_rows_d || !out_scores_d || !out_rows_d)
    return api_fail(RFX_EINVAL, "lex fuse: null lists / outputs");
  std::lock_guard<std::mutex> lk(lx->mu);
  LEX_HIP(hipSetDevice(lx->device));
  hipStream_t st = (hipStream_t)stream;
  // The per-question tables {alpha, n_dense, n_lex} through pinned staging to the handle's device tables
  // (stream-ordered: the caller's arrays may die on return).
  const size_t tab = al256((size_t)nq * 4);
  if (const int rc = stage_acquire(*lx, 3 * tab)) return rc;
  uint8_t* s8 = (uint8_t*)lx->stage;
  for (int64_t q = 0; q < nq; ++q) {
    ((float*)s8)[q] = alpha_h ? alpha_h[q] : 0.5f;
    ((int32_t*)(s8 + tab))[q] = n_dense_h ? n_dense_h[q] : n_dense_max;
    ((int32_t*)(s8 + 2 * tab))[q] = n_lex_h ? n_lex_h[q] : n_lex_max;
  }
  if (!lx->fuse_tab && hipMalloc(&lx->fuse_tab, 3 * al256((size_t)rfx::kLexMaxNq * 4)) != hipSuccess)
    return api_fail(RFX_ENOMEM, "hipMalloc failed (fusion tables)");
  uint8_t* t_d = (uint8_t*)lx->fuse_tab;
  LEX_HIP(hipMemcpyAsync(t_d, s8, 3 * tab, hipMemcpyHostToDevice, st));
  const int rc = rfx::launch_rrf_fuse(dense_rows_d, n_dense_max, lex_rows_d, n_lex_max, nq, k, (const float*)t_d,
                                      (const int32_t*)(t_d + tab), (const int32_t*)(t_d + 2 * tab), rrf_c, out_scores_d,
                                      out_rows_d, out_ranks_d, st);
  // recorded after the kernel: the next user of the staging buffer or of the device tables waits for both
  LEX_HIP(hipEventRecord(lx->stage_ev, st));
  if (rc != 0) return api_fail(RFX_EUNSUPPORTED, "lex fuse launch rejected");
  LEX_HIP(hipGetLastError());
  return RFX_OK;
}

}  // extern "C"
