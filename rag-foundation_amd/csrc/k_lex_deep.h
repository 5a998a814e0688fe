// k_lex_deep.h — the BM25 lexical scan at depth: top-k for k in 65..1,024 (rfx_lex_search_deep).
// Host-side plan and launchers; kernels: k_lex_deep.hip.  Scores: k_lex_score.h, the bits of rfx_lex_search.
//
// Path: the retrieval slice of ask_stream (gemini_rag.py:517-551) at the depth a rank fusion or a re-ranker reads.
//
// A candidate is one u64 key, cand_key of k_cand_keys.h; a BM25 score that ranks is > 0, so its key is never 0.
//
// lex_deep_scan_kernel<NQT, LDS>: grid (blocks, groups), 1,024 threads, lex_scan_kernel's tile walk.  A group is
// 4 questions (1 for a lone question): the weight table w[V][4] takes 64 KB at V 4,096 and leaves LDS for the
// selection.  Per question LDS holds a buffer of CAP = max(1,024, 2 KB) keys, a fill counter and a threshold key
// tau.  A row's key enters the buffer when it beats tau (full-key compare: the waves of a workgroup do not visit
// rows in ascending order).  The workgroup walks the tiles in rounds, one 32-row tile per wave, so a round adds
// at most kLexDeepRound = 512 keys to a buffer; it meets after every round and cuts every buffer whose fill has
// passed CAP - 512 (sort, keep KB, tau = the KB-th key).  A buffer therefore starts every round with room for
// the whole round: it cannot overflow, and there is no other path.  At the end each buffer is cut once more and
// its KB keys go to slab[q][block * KB ..); launch_deep_select (k_deep_select.h) picks each question's k best of them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "deep_plan.h"
#include "k_lex.h"

namespace rfx {

constexpr int kLexDeepGroup = 4;      // questions per weight table
constexpr int kLexDeepRound = 512;    // keys a round can add to one buffer: 16 waves x one 32-row tile
constexpr int kLexDeepTargetWgs = 512;

struct LexDeepPlan {
  int nqt;     // questions per group: 1 (a lone question) or 4
  int groups;  // grid.y
  int blocks;  // grid.x = runs of KB keys per question in the slab
  int kb;      // deep_kb(k): keys a buffer keeps at a cut
  int cap;     // keys a buffer holds: max(1024, 2 kb); kb <= cap - kLexDeepRound
  bool lds;    // weight table staged in LDS (V <= kLexLdsV)
};
// block_cap > 0 caps the blocks (RFX_LEX_DEEP_BLOCKS)
LexDeepPlan lex_deep_plan(int64_t rows, int V, int64_t nq, int k, int block_cap);

// The scan: slab [nq][blocks * kb] keys (0 = none) and n_keys [nq] = blocks * kb.  W: launch_lex_weights' tables at
// nqt questions per group.  -1: arguments outside the kernel's range.
int launch_lex_deep_scan(const LexDeepPlan& p, int V, const int64_t* indptr, const uint32_t* entries, const int32_t* len,
                         int64_t rows, const float* W, int64_t nq, double k1, double b, double avgdl,
                         const uint32_t* mask, uint64_t* slab, int* n_keys, hipStream_t st);
// scores / rows [n] <- (-inf, -1): the answer of an index without a live row
void launch_lex_deep_none(float* scores, int64_t* rows, int64_t n, hipStream_t st);

}  // namespace rfx
