// k_lex.h — the BM25 lexical scan (rfx_lex_search).  Host-side launchers; kernels: k_lex.hip.
//
// Path: the retrieval slice of ask_stream (gemini_rag.py:517-551), a keyword signal beside the dense one.
// Store layout (lex_host.h): indptr int64 [rows + 1], one packed u32 per entry (bucket | tf << 16, sorted by
// bucket within a row), len int32 [rows] (-1 = dead).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lex_host.h"

namespace rfx {

constexpr int kLexThreads = 1024;         // 16 waves: the 128 KB weight table leaves one workgroup per CU
constexpr int kLexBlocks = 256;           // one per CU
constexpr int kLexLdsV = 4096;            // the weight table lives in LDS up to this V (8 questions: 128 KB)

struct LexPlan {
  int nqt;      // questions per group: 1 (a lone question) or 8
  int groups;   // grid.y
  int blocks;   // grid.x = candidate lists per question
  int k_slot;   // list length: 4 / 16 / 64
  bool lds;     // weight table staged in LDS (V <= kLexLdsV), else read from L2
};
LexPlan lex_plan(int64_t rows, int V, int64_t nq, int k);

// dense weight tables W[groups][V][nqt] (f32), zeroed then filled from the sparse question entries
// (q_off [nq + 1], q_ent [q_off[nq]]): one launch
void launch_lex_weights(const LexPlan& p, int V, const int32_t* q_off, const LexQueryEntry* q_ent, int64_t nq, float* W,
                        hipStream_t st);
// the scan: cs / cr [nq][blocks][k_slot] sorted candidate lists (empty slots (-inf, kEmptyRow))
int launch_lex_scan(const LexPlan& p, int V, const int64_t* indptr, const uint32_t* entries, const int32_t* len,
                    int64_t rows, const float* W, int64_t nq, double k1, double b, double avgdl, const uint32_t* mask,
                    float* cs, int* cr, hipStream_t st);
void launch_lex_set_dead(int32_t* len, const int64_t* rows_d, int64_t n, hipStream_t st);

}  // namespace rfx
