"""GpuRetriever — the index-write / search engine behind LocalGpuRag.

Every call goes to the HIP library (librfx.so); there is no CPU path.
"""
import collections
import os
import threading
from dataclasses import dataclass

import torch

from . import filters
from .batcher import GroupBatcher
from .distinct import DISTINCT_ERROR, parse_distinct
from .embedder import DEFAULT_MAX_TOKENS, DEFAULT_OVERLAP, Embedder, featurize_texts
from .store import ivf_filtered_mode, ivf_multi_mode, registry as default_registry
from . import union as runion


@dataclass
class Hit:
    score: float
    store: str
    row: int
    file_id: str
    text: str
    title: str
    uri: str


def _chunking(cfg):
    """Gemini chunking_config -> (max_tokens, overlap); defaults when absent."""
    if not cfg:
        return DEFAULT_MAX_TOKENS, DEFAULT_OVERLAP
    ws = cfg.get("white_space_config", cfg) if isinstance(cfg, dict) else {}
    mt = int(ws.get("max_tokens_per_chunk", DEFAULT_MAX_TOKENS))
    ov = int(ws.get("max_overlap_tokens", DEFAULT_OVERLAP))
    return mt, min(ov, mt - 1)


# Process-wide state: get_rag_client() builds a new adapter (and retriever) per request
# (chat.py:937, ingestion.py:214), so embedders and batchers live at module level — one per
# (device, dim) and per store — or no two requests would ever share a batch.
_STATE_LOCK = threading.Lock()
_EMBEDDERS = {}
_BATCHERS = {}  # (store name | tuple of names, filter key | _FILTERED, registry id) -> GroupBatcher
_FILTERED = "\x00filtered"  # the one batcher of a store's filtered questions (no filter_key starts with NUL)
# (tuple of names, registry id) -> UnionView (rfx.union), least recently used first; it follows its
# members' appends and tombstones in place.  Bounded in device bytes (RFX_UNION_MAX_BYTES, default
# 32 GiB): the least recently used views are evicted, and a view over its own budget is not built
# (that question takes the per-store path).  A view in use when evicted is closed by its last user.
_UNIONS = collections.OrderedDict()
_UNION_BYTES = [0]


def union_budget() -> int:
    return int(os.environ.get("RFX_UNION_MAX_BYTES", str(32 << 30)))


def segmented_mode() -> str:
    """RFX_SEGMENTED: "0" = one masked search per distinct filter (a batcher per (store, filter)), "1" = the
    segmented search for every filtered batch, "auto" (default) = by segmented_max_fraction's rule.  Read at
    every question: services and tests may change it."""
    m = os.environ.get("RFX_SEGMENTED", "auto").strip().lower()
    return m if m in ("0", "1") else "auto"


def segmented_max_fraction() -> float:
    """F of the auto rule (RFX_SEGMENTED_MAX_FRACTION): a filtered batch takes the segmented search when
    sum over filters of (selected rows x ceil(questions / 8)) <= F x distinct filters x store rows, i.e. when
    the rows it would read are at most F of what one masked search per filter reads.  Default: the largest
    swept fraction at which the segmented batch was still the faster one, rounded down to a power of two
    (tools/bench_filters.py)."""
    return float(os.environ.get("RFX_SEGMENTED_MAX_FRACTION", "0.5"))


DIVERSITY_ERROR = "diversity needs a flat single-device store"


def default_fetch_k(k: int) -> int:
    """Candidates a diversified question fetches when it names no fetch_k: min(64, max(4k, 16))."""
    return min(64, max(4 * int(k), 16))


def parse_diversity(diversity, k: int):
    """diversity (None | lambda | {"lambda": .., "fetch_k": ..}) -> None or (lambda, fetch_k) with
    0 <= lambda <= 1 and k <= fetch_k <= 64 (MMR over the fetch_k best rows)."""
    if diversity is None:
        return None
    if isinstance(diversity, dict):
        unknown = set(diversity) - {"lambda", "fetch_k"}
        if unknown or "lambda" not in diversity:
            raise ValueError(f"diversity takes 'lambda' and optionally 'fetch_k', got {sorted(diversity)}")
        lam, fetch_k = diversity["lambda"], diversity.get("fetch_k")
    else:
        lam, fetch_k = diversity, None
    if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not 0.0 <= float(lam) <= 1.0:
        raise ValueError(f"diversity lambda={lam!r} must be a number in [0, 1]")
    fetch_k = default_fetch_k(k) if fetch_k is None else int(fetch_k)
    if not k <= fetch_k <= 64:
        raise ValueError(f"diversity fetch_k={fetch_k} must satisfy k={k} <= fetch_k <= 64")
    return float(lam), fetch_k


HYBRID_ERROR = "hybrid needs a flat single-device store and no diversity"
_HYBRID = "\x00hybrid"  # tag of a store's hybrid batchers (no filter_key starts with NUL)


def parse_hybrid(hybrid, k: int):
    """hybrid (None | alpha | {"alpha": .., "fetch_k": .., "rrf_c": .., "k1": .., "b": ..}) -> None or
    (alpha, fetch_k, rrf_c, k1, b): reciprocal-rank fusion of the dense and the BM25 answer at fetch_k each
    (DESIGN §4.14).  0 <= alpha <= 1 (1 = dense only), k <= fetch_k <= 64 (default default_fetch_k(k)),
    rrf_c >= 1 (60), k1 >= 0 (1.2), 0 <= b <= 1 (0.75)."""
    if hybrid is None:
        return None
    if isinstance(hybrid, dict):
        unknown = set(hybrid) - {"alpha", "fetch_k", "rrf_c", "k1", "b"}
        if unknown or "alpha" not in hybrid:
            raise ValueError(f"hybrid takes 'alpha' and optionally 'fetch_k', 'rrf_c', 'k1', 'b', got {sorted(hybrid)}")
        opts = hybrid
    else:
        opts = {"alpha": hybrid}

    def number(name, default, lo, hi):
        v = opts.get(name, default)
        if v is None:
            v = default
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not lo <= float(v) <= hi:  # (a NaN fails)
            raise ValueError(f"hybrid {name}={v!r} must be a number in [{lo}, {hi}]")
        return float(v)

    alpha = number("alpha", None, 0.0, 1.0)
    k1 = number("k1", 1.2, 0.0, 3.0e38)
    b = number("b", 0.75, 0.0, 1.0)
    fetch_k, rrf_c = opts.get("fetch_k"), opts.get("rrf_c", 60)
    for name, v in (("fetch_k", fetch_k), ("rrf_c", rrf_c)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, int)):
            raise ValueError(f"hybrid {name}={v!r} must be an integer")
    fetch_k = default_fetch_k(k) if fetch_k is None else int(fetch_k)
    if not k <= fetch_k <= 64:
        raise ValueError(f"hybrid fetch_k={fetch_k} must satisfy k={k} <= fetch_k <= 64")
    rrf_c = 60 if rrf_c is None else int(rrf_c)
    if not 1 <= rrf_c <= 2 ** 31 - 1:
        raise ValueError(f"hybrid rrf_c={rrf_c} must be an integer >= 1")
    return alpha, fetch_k, rrf_c, k1, b


_DISTINCT = "\x00distinct"  # tag of a store's distinct-document batchers (no filter_key starts with NUL)


def _distinct_ok(st) -> bool:
    """A flat store on one device whose index runs the distinct-document search (DeviceIndex.search_distinct)
    and which knows its rows' documents (LocalStore.row_docs)."""
    return hasattr(st.index, "search_distinct") and hasattr(st, "row_docs") and \
        getattr(st, "spec", {}).get("kind", "flat") == "flat"


def _diversity_ok(st) -> bool:
    """A flat store on one device: its index selects on the device (DeviceIndex.mmr_select) and no IVF
    lists answer in its place."""
    return hasattr(st.index, "mmr_select") and getattr(st, "spec", {}).get("kind", "flat") == "flat"


def _search_diverse(index, q, items, div_at, row_mask=None):
    """The batch's search at its largest fetch_k (k for the items that asked for no diversity), then ONE
    MMR selection over the batch: lambda 1 and n_cand = k for the items without, their own lambda and
    fetch_k otherwise.  items[i][1] = k, items[i][div_at] (when present) = (lambda, fetch_k).  Returns
    host lists (scores, rows) [nq][largest k]."""
    divs = [it[div_at] if len(it) > div_at else None for it in items]
    ks = [it[1] for it in items]
    fetch = max(d[1] if d else k for d, k in zip(divs, ks))
    s, r = index.search(q, fetch, row_mask=row_mask)
    s, r = index.mmr_select(q, s, r, max(ks), lam=[d[0] if d else 1.0 for d in divs],
                            n_cand=[d[1] if d else k for d, k in zip(divs, ks)])
    return s.cpu(), r.cpu()


class _StoreAnswer(tuple):
    """(store, scores, rows) of one question, plus .generation: the store generation whose row numbering
    `rows` uses (LocalStore.row_info translates or refuses rows of an earlier one after a compaction)."""
    generation = None


def _answer(st, s, r, generation):
    a = _StoreAnswer((st, s, r))
    a.generation = generation
    return a


def _numbered(st, fn):
    """fn() -> result, run under one row numbering of `st`: (result, generation).  A compaction that
    renumbers the store's rows while fn resolves masks or ranges and searches makes it run again."""
    if not hasattr(st, "numbering"):
        return fn(), None
    while True:
        token, generation = st.numbering()
        out = fn()
        if not st.numbering_changed(token):
            return out, generation


def _evict_union(key, closing):
    """(caller holds _STATE_LOCK) Drop the view from the cache; an unpinned view goes to `closing`, which the
    caller closes after releasing the lock.  Its bytes stay counted until it is closed (a pinned view's
    device memory lives until its last user releases it: ADVICE r4)."""
    v = _UNIONS.pop(key)
    v.evicted = True
    if v.users == 0:
        closing.append(v)


def _close_unions(closing):
    """Close evicted views outside _STATE_LOCK (hipFree may wait for the device), then uncount them."""
    nbytes = sum(v.nbytes for v in closing)
    for v in closing:
        v.close()
    if closing:
        with _STATE_LOCK:
            _UNION_BYTES[0] -= nbytes


def _release_union(v):
    closing = []
    with _STATE_LOCK:
        v.users -= 1
        if v.evicted and v.users == 0:
            closing.append(v)
    _close_unions(closing)


def _purge_batchers(name):
    closing = []
    with _STATE_LOCK:
        for key in [k for k in _BATCHERS if k[0] == name or (isinstance(k[0], tuple) and name in k[0])]:
            del _BATCHERS[key]
        for key in [k for k in _UNIONS if name in k[0]]:
            _evict_union(key, closing)
    _close_unions(closing)


class GpuRetriever:
    def __init__(self, registry=None, dim=None, dtype=None):
        self._registry = registry
        self.dim = int(os.environ.get("RFX_DIM", "768")) if dim is None else int(dim)
        # bf16 stores by default: half the HBM bytes of f32, and the bf16 MFMA scans run 8x the f32
        # matrix rate.  An f32 store's micro-batches of more than 16 questions run kernel 9 (f32
        # MFMA, one corpus pass per 128 queries); smaller ones the VALU scan in 8-query slices.
        # Parity is defined on the stored values (the oracle widens stored rows exactly), so bf16
        # loses nothing against it; RFX_DTYPE=f32 keeps full-precision vectors where the
        # application wants them.
        self.dtype = os.environ.get("RFX_DTYPE", "bf16") if dtype is None else dtype
        # micro-batching of concurrent questions per store (RFX_BATCH=0 disables)
        self.batching = os.environ.get("RFX_BATCH", "1") != "0"
        # a question over several stores: one scan of their union (rfx.union; RFX_UNION=0 disables)
        self.union = os.environ.get("RFX_UNION", "1") != "0"
        self.last_path = None  # "union" | "per-store" (tests, diagnostics)
        self.last_filter_path = None  # "segmented" | "masked" | "ivf": how the last filtered batch was searched
        self.last_filter_list_searches = 0  # list searches the last filtered batch issued (IVF stores, §4.16)
        self.last_diversity = None  # "union" | "store" | None: where the last question was diversified
        self.last_hybrid = None  # "store" | None: the last question fused a dense and a lexical answer per store
        self.last_distinct_rounds = None  # rounds of the last distinct-document batch (1 = the first search sufficed)

    @property
    def registry(self):
        return self._registry or default_registry()

    def embedder(self, dim) -> Embedder:
        key = (self.registry.device, dim)
        with _STATE_LOCK:
            e = _EMBEDDERS.get(key)
            if e is None:
                e = Embedder(dim=dim, device=self.registry.device)
                _EMBEDDERS[key] = e
            return e

    # ---- store namespace ----------------------------------------------------------------------
    def create_store(self, display_name):
        return self.registry.create(display_name, self.dim, self.dtype).name

    def drop_store(self, name):
        _purge_batchers(name)
        return self.registry.drop(name)

    def store_names(self):
        return self.registry.names()

    # ---- index write --------------------------------------------------------------------------
    def add_document(self, store_name, text, display_name, chunking_config=None, metadata=None):
        st = self.registry.get(store_name)
        if st is None:
            raise ValueError(f"unknown store {store_name!r}")
        mt, ov = _chunking(chunking_config)
        with torch.cuda.device(st.device):
            chunks, vecs = self.embedder(st.dim).chunk_and_embed(text, st.dtype, mt, ov)
            file_id, _ = st.add_document(chunks, vecs, display_name, metadata)
        return file_id, len(chunks)

    def delete_file(self, store_name, file_id):
        st = self.registry.get(store_name)
        return bool(st and st.delete_file(file_id))

    def compact_store(self, name):
        """Rewrite the store without the rows of its deleted documents (LocalStore.compact):
        {"rows_before", "rows", "seconds"}.  ValueError for an unknown store."""
        st = self.registry.get(name)
        if st is None:
            raise ValueError(f"unknown store {name!r}")
        with torch.cuda.device(st.device):
            return st.compact()

    # ---- retrieval ----------------------------------------------------------------------------
    def _search_store_batch(self, st, items, row_mask=None):
        """One GPU search for a batch of (question, k) against one store: one embedding GEMM,
        one scan + merge at the largest k; each item gets its own first k."""
        if any(len(it) > 2 for it in items):  # some ask for diversity: (question, k, (lambda, fetch_k))
            if not _diversity_ok(st):
                raise ValueError(DIVERSITY_ERROR)
            with torch.cuda.device(st.device):
                q = self.embedder(st.dim).embed_texts([it[0] for it in items], st.dtype)
                s, r = _search_diverse(st.index, q, items, 2, row_mask)
                s, r = s.tolist(), r.tolist()
            return [(s[i][:it[1]], r[i][:it[1]]) for i, it in enumerate(items)]
        kmax = max(k for _, k in items)
        with torch.cuda.device(st.device):
            q = self.embedder(st.dim).embed_texts([t for t, _ in items], st.dtype)
            s, r = st.search(q, kmax, row_mask=row_mask)
            s, r = s.cpu().tolist(), r.cpu().tolist()
        return [(s[i][:k], r[i][:k]) for i, (_, k) in enumerate(items)]

    @staticmethod
    def _lists_possible(st) -> bool:
        """RFX_IVF_FILTERED is on and the store has posting lists: its rule may send a plain filtered
        question there (LocalStore.search_lists_filtered decides, per filter, when it runs)."""
        return getattr(st, "ivf", None) is not None and hasattr(st, "search_lists_filtered") and \
            ivf_filtered_mode() != "0"

    def _run_batch(self, name, metadata_filter, items):
        """Batch runner: resolves the store and its row mask when the batch runs (a batcher holds
        no LocalStore, so a store that another process replaced or dropped is freed here too).
        A filtered batch of plain questions (none asks for diversity) takes an IVF store's posting lists
        when the store's rule says so (RFX_IVF_FILTERED; LocalStore.search_filtered reports the path);
        filtered diverse, hybrid and union-view questions keep the exact scan."""
        st = self.registry.get(name)
        if st is None:
            return [None] * len(items)
        path = ["masked"]
        def run():
            mask = st.row_mask(metadata_filter) if metadata_filter is not None else None
            if metadata_filter is not None and mask is None:
                return None
            path[0] = "masked"
            if mask is not None and all(len(it) == 2 for it in items) and self._lists_possible(st):
                kmax = max(k for _, k in items)
                with torch.cuda.device(st.device):
                    q = self.embedder(st.dim).embed_texts([t for t, _ in items], st.dtype)
                    s, r, p = st.search_filtered(q, kmax, metadata_filter)  # (the exact path = the masked search)
                    s, r = s.tolist(), r.tolist()
                path[0] = "ivf" if p == "ivf" else "masked"
                return [(s[i][:k], r[i][:k]) for i, (_, k) in enumerate(items)]
            return self._search_store_batch(st, items, mask)

        res, gen = _numbered(st, run)
        if res is None:
            return [None] * len(items)
        if metadata_filter is not None:
            self.last_filter_path = path[0]
        return [_answer(st, s, r, gen) for s, r in res]

    def _run_hybrid_batch(self, name, metadata_filter, items):
        """Batch runner of a store's hybrid questions, items (question, k, (alpha, fetch_k, rrf_c, k1, b)) that
        share rrf_c, k1 and b (the batcher's key): one embedding, one dense search at the largest fetch_k, one
        featurisation of the questions, one BM25 search at the same fetch_k, one fusion with each item's own
        alpha and list lengths; each item takes its first k.  A filter's row mask applies to both searches."""
        st = self.registry.get(name)
        if st is None:
            return [None] * len(items)
        if not _diversity_ok(st):
            raise ValueError(HYBRID_ERROR)
        _, _, rrf_c, k1, b = items[0][2]
        fetch = max(it[2][1] for it in items)
        kmax = max(it[1] for it in items)

        def run():
            mask = st.row_mask(metadata_filter) if metadata_filter is not None else None
            if metadata_filter is not None and mask is None:
                return None
            with torch.cuda.device(st.device), st.lock:  # no append moves either index between the two searches
                lex = st.lexical()
                csr = featurize_texts([it[0] for it in items], lex.V, lex.hash_seed)
                q = self.embedder(st.dim).embed_csr(*csr, dtype=st.dtype)
                _, rd = st.index.search(q, fetch, row_mask=mask)
                _, rl = lex.search(csr, fetch, k1=k1, b=b, row_mask=mask)
                n = [it[2][1] for it in items]
                s, r = lex.fuse(rd, rl, kmax, [it[2][0] for it in items], n_dense=n, n_lex=n, rrf_c=rrf_c)
                s, r = s.cpu().tolist(), r.cpu().tolist()
            return [(s[i][:it[1]], r[i][:it[1]]) for i, it in enumerate(items)]

        res, gen = _numbered(st, run)
        if res is None:
            return [None] * len(items)
        return [_answer(st, s, r, gen) for s, r in res]

    def _hybrid_batcher(self, name, metadata_filter, hyb):
        # hybrid questions of a store ride batchers of their own: the existing key with a hybrid tag (and the
        # parameters one launch shares), so no existing batch ever changes shape
        tag = f"{_HYBRID}:{hyb[2]}:{hyb[3]!r}:{hyb[4]!r}:{filters.filter_key(metadata_filter)}"
        key = (name, tag, id(self.registry))
        with _STATE_LOCK:
            b = _BATCHERS.get(key)
            if b is None:
                if self.registry.on_evict.count(_purge_batchers) == 0:
                    self.registry.on_evict.append(_purge_batchers)
                b = GroupBatcher(lambda items, n=name, f=metadata_filter: self._run_hybrid_batch(n, f, items),
                                 max_batch=256)
                if len(_BATCHERS) >= 4096:
                    _BATCHERS.clear()
                _BATCHERS[key] = b
            return b

    def _run_distinct_batch(self, name, metadata_filter, items):
        """Batch runner of a store's distinct-document questions, items (question, k, fetch_k): one embedding,
        then DeviceIndex.search_distinct at the largest k and the largest fetch_k (the answer is exact at any
        fetch_k, and the first k of the rule's answer at a larger k is its answer at k); each item takes its
        first k.  A filter applies as the row mask of round 1 and as the select ranges of the completion.  The
        whole batch runs under the store's lock and one row numbering: no append, delete or compaction moves
        the rows or their documents between the rounds."""
        st = self.registry.get(name)
        if st is None:
            return [None] * len(items)
        if not _distinct_ok(st):
            raise ValueError(DISTINCT_ERROR)
        kmax = max(it[1] for it in items)
        fetch = max(it[2] for it in items)
        rounds = [None]

        def run():
            with torch.cuda.device(st.device), st.lock:
                mask = st.row_mask(metadata_filter) if metadata_filter is not None else None
                if metadata_filter is not None and mask is None:
                    return None
                sel = st.segment_ranges(metadata_filter) if metadata_filter is not None else None
                row_doc, doc_ranges, _ = st.row_docs()
                q = self.embedder(st.dim).embed_texts([it[0] for it in items], st.dtype)
                s, r, _, rounds[0] = st.index.search_distinct(q, kmax, row_doc, doc_ranges, fetch_k=fetch,
                                                              row_mask=mask, select_ranges=sel)
                s, r = s.cpu().tolist(), r.cpu().tolist()
            return [(s[i][:it[1]], r[i][:it[1]]) for i, it in enumerate(items)]

        res, gen = _numbered(st, run)
        if res is None:
            return [None] * len(items)
        self.last_distinct_rounds = rounds[0]
        return [_answer(st, s, r, gen) for s, r in res]

    def _distinct_batcher(self, name, metadata_filter):
        # distinct questions of a store ride batchers of their own, keyed like the hybrid ones (store, a distinct
        # tag, the filter's key): no existing batch ever changes shape
        key = (name, f"{_DISTINCT}:{filters.filter_key(metadata_filter)}", id(self.registry))
        with _STATE_LOCK:
            b = _BATCHERS.get(key)
            if b is None:
                if self.registry.on_evict.count(_purge_batchers) == 0:
                    self.registry.on_evict.append(_purge_batchers)
                b = GroupBatcher(lambda items, n=name, f=metadata_filter: self._run_distinct_batch(n, f, items),
                                 max_batch=256)
                if len(_BATCHERS) >= 4096:
                    _BATCHERS.clear()
                _BATCHERS[key] = b
            return b

    def _run_filtered_batch(self, name, items):
        """Batch runner of a store's filtered questions, items (question, k, filter): the items are grouped
        by filter and each group's row ranges resolved (a filter that matches no file answers None); then
        ONE segmented search reads only the selected rows (DeviceIndex.search_segmented), or, when the
        filters select too much of the store for that to pay (segmented_max_fraction), one masked search
        per distinct filter runs as before.  On an IVF store under RFX_IVF_FILTERED, a group of plain
        questions (no diversity) whose filter the store's rule sends to the posting lists is answered
        there first (last_filter_path "ivf") — two or more such groups in ONE list search at the batch's
        largest k (LocalStore.search_lists_filtered_multi; a lone group, and every group under
        RFX_IVF_MULTI=0, takes the one-mask search of §4.15, one per group;
        last_filter_list_searches counts them); every other group goes through the choice above unchanged.
        Filtered diverse, hybrid and union-view questions keep the exact scan."""
        st = self.registry.get(name)
        if st is None:
            return [None] * len(items)
        out, gen = _numbered(st, lambda: self._filtered_batch(st, items))
        return [None if o is None else _answer(*o, gen) for o in out]

    def _filtered_batch(self, st, items):
        out = [None] * len(items)
        groups = []  # (filter, item indices, ranges) of the filters that select rows
        diverse = any(len(it) > 3 for it in items)  # (question, k, filter, (lambda, fetch_k))
        if diverse and not _diversity_ok(st):
            raise ValueError(DIVERSITY_ERROR)
        for filt, idxs in filters.group_by_filter([it[2] for it in items]):
            ranges = st.segment_ranges(filt)
            if ranges:
                groups.append((filt, idxs, ranges))
        rest = groups
        self.last_filter_list_searches = 0
        if self._lists_possible(st):  # plain groups the store's rule sends to its posting lists
            plain = [g for g in groups if all(len(items[i]) == 3 for i in g[1])]
            rest = [g for g in groups if not all(len(items[i]) == 3 for i in g[1])]
            if plain:
                order = [i for _, idxs, _ in plain for i in idxs]
                at = {i: p for p, i in enumerate(order)}
                # one plain group is the one-mask search it always was (the per-question entry point costs a table
                # upload and a launch more per call); two or more share ONE list search
                multi = ivf_multi_mode() and len(plain) > 1
                with torch.cuda.device(st.device):  # one embedding for all of them
                    q_all = self.embedder(st.dim).embed_texts([items[i][0] for i in order], st.dtype)
                    if multi:  # ONE list search for every group the rule sends to the lists, at the batch's k
                        kmax = max(items[i][1] for i in order)
                        res = st.search_lists_filtered_multi(q_all, kmax, [items[i][2] for i in order])
                        declined = set(range(len(order))) if res is None else set(res[2])
                        rest += [g for g in plain if at[g[1][0]] in declined]
                        if res is not None:
                            self.last_filter_path = "ivf"
                            self.last_filter_list_searches += 1
                            s, r = res[0].tolist(), res[1].tolist()
                            for i in order:
                                if at[i] not in declined:
                                    out[i] = (st, s[at[i]][:items[i][1]], r[at[i]][:items[i][1]])
                    for g in ([] if multi else plain):
                        filt, idxs, _ = g
                        q = q_all[[at[i] for i in idxs]].contiguous()
                        res = st.search_lists_filtered(q, max(items[i][1] for i in idxs), filt)
                        if res is None:  # the rule keeps this filter exact: the choice below, as ever
                            rest.append(g)
                            continue
                        self.last_filter_path = "ivf"
                        self.last_filter_list_searches += 1
                        s, r = res[0].tolist(), res[1].tolist()
                        for p, i in enumerate(idxs):
                            out[i] = (st, s[p][:items[i][1]], r[p][:items[i][1]])
        groups = rest
        if not groups:
            return out
        mode = segmented_mode()
        if mode == "auto":
            cost = sum(sum(n for _, n in ranges) * ((len(idxs) + 7) // 8) for _, idxs, ranges in groups)
            mode = "1" if cost <= segmented_max_fraction() * len(groups) * st.index.rows else "0"
        if mode == "0":
            self.last_filter_path = "masked"
            for filt, idxs, _ in groups:
                mask = st.row_mask(filt)
                if mask is None:
                    continue
                res = self._search_store_batch(st, [items[i][:2] + items[i][3:] for i in idxs], mask)
                for i, (s, r) in zip(idxs, res):
                    out[i] = (st, s, r)
            return out
        self.last_filter_path = "segmented"
        live = [i for _, idxs, _ in groups for i in idxs]
        pos = {i: p for p, i in enumerate(live)}
        kmax = max(items[i][1] for i in live)
        if diverse:  # the segmented search at the largest fetch_k, then one selection over the batch
            divs = [items[i][3] if len(items[i]) > 3 else None for i in live]
            ks = [items[i][1] for i in live]
            fetch = max(d[1] if d else k for d, k in zip(divs, ks))
        with torch.cuda.device(st.device):
            q = self.embedder(st.dim).embed_texts([items[i][0] for i in live], st.dtype)
            seg = [([pos[i] for i in idxs], ranges) for _, idxs, ranges in groups]
            if diverse:
                s, r = st.index.search_segmented(q, fetch, seg)
                s, r = st.index.mmr_select(q, s, r, kmax, lam=[d[0] if d else 1.0 for d in divs],
                                           n_cand=[d[1] if d else k for d, k in zip(divs, ks)])
            else:
                s, r = st.index.search_segmented(q, kmax, seg)
            s, r = s.cpu().tolist(), r.cpu().tolist()
        for i in live:
            k = items[i][1]
            out[i] = (st, s[pos[i]][:k], r[pos[i]][:k])
        return out

    def _batcher(self, name, metadata_filter, shared=False):
        # masked searches: one batcher per (store, filter), a launch applies one row mask to all its queries;
        # shared: the store's ONE batcher of filtered questions (items carry their filter: _run_filtered_batch)
        key = (name, _FILTERED if shared else filters.filter_key(metadata_filter), id(self.registry))
        with _STATE_LOCK:
            b = _BATCHERS.get(key)
            if b is None:
                if self.registry.on_evict.count(_purge_batchers) == 0:
                    self.registry.on_evict.append(_purge_batchers)
                if shared:
                    b = GroupBatcher(lambda items, n=name: self._run_filtered_batch(n, items), max_batch=256)
                else:
                    b = GroupBatcher(lambda items, n=name, f=metadata_filter: self._run_batch(n, f, items),
                                     max_batch=256)
                if len(_BATCHERS) >= 4096:
                    _BATCHERS.clear()
                _BATCHERS[key] = b
            return b

    def _segmentable(self, name):
        """Filtered questions of this store go through the shared batcher: a single-device flat index
        (sharded stores keep one masked search per filter), unless RFX_SEGMENTED=0."""
        if segmented_mode() == "0":
            return False
        st = self.registry.get(name)
        return st is not None and hasattr(st.index, "search_segmented") and hasattr(st, "segment_ranges")

    def search_store(self, name, question, k, metadata_filter=None, diversity=None, hybrid=None, distinct=None):
        """(store, scores, rows) of one question against one store, or None when the store is
        gone or the filter selects no row of it; batched with concurrent callers of the same
        store (filtered questions of a store share one batch, whatever their filters).
        hybrid: parse_hybrid's tuple; the scores are then the fused ones (masked path under a filter).
        distinct: parse_distinct's fetch_k; the rows are then the best chunks of k different files."""
        if distinct is not None:
            if diversity or hybrid is not None:
                raise ValueError(DISTINCT_ERROR)
            item = (question, int(k), int(distinct))
            if self.batching:
                return self._distinct_batcher(name, metadata_filter).submit(item)
            return self._run_distinct_batch(name, metadata_filter, [item])[0]
        if hybrid is not None:
            if diversity:
                raise ValueError(HYBRID_ERROR)
            item = (question, int(k), tuple(hybrid))
            if self.batching:
                return self._hybrid_batcher(name, metadata_filter, hybrid).submit(item)
            return self._run_hybrid_batch(name, metadata_filter, [item])[0]
        if metadata_filter is not None and self._segmentable(name):
            item = (question, int(k), metadata_filter) + ((diversity,) if diversity else ())
            if self.batching:
                return self._batcher(name, None, shared=True).submit(item)
            return self._run_filtered_batch(name, [item])[0]
        item = (question, int(k)) + ((diversity,) if diversity else ())
        if self.batching:
            return self._batcher(name, metadata_filter).submit(item)
        return self._run_batch(name, metadata_filter, [item])[0]

    # ---- several stores in one launch (rfx.union) ------------------------------------------------
    def _union_view(self, names, stores):
        """The cached view over `stores` brought up to date (in place when the members only grew or
        deleted rows), pinned for the caller (_release_union), or None when a view of this size does not
        fit the cache's byte budget.  Callers hold every member's lock.

        The device copies (a view's build, a follow's appended rows) run OUTSIDE _STATE_LOCK (VERDICT r4
        #7): that lock guards the cache's dict and counters only, and every batcher, embedder and union
        lookup of the process takes it, so a copy under it would stall every chat thread.  What serialises
        the copies is the member locks the caller holds: every user of a view holds all of its members'
        locks (the key is the member list), so no other thread searches or follows this view meanwhile."""
        key = (tuple(names), id(self.registry))
        want = runion.union_key(stores)
        closing = []
        with _STATE_LOCK:
            v = _UNIONS.get(key)
            if v is not None:
                _UNIONS.move_to_end(key)
                v.users += 1  # pinned: an eviction meanwhile leaves it open for us
        if v is not None:
            ok = v.key == want
            if not ok:
                try:
                    ok = v.follow(stores)
                except BaseException:
                    _release_union(v)
                    raise
            if ok:
                return v
            with _STATE_LOCK:
                if _UNIONS.get(key) is v:
                    _evict_union(key, closing)
            _release_union(v)
        _close_unions(closing)
        closing = []
        need, budget = runion.planned_bytes(stores), union_budget()
        if need > budget:
            return None
        with _STATE_LOCK:  # room for it (bytes reserved while it is built)
            # an evicted view stays counted until _close_unions uncounts it (after the lock), so the loop
            # keeps its own tally of what the evictions free: only the least recently used views that make
            # room go.  A pinned view frees nothing until its last user releases it.
            freed = 0
            while _UNIONS and _UNION_BYTES[0] - freed + need > budget:
                n0 = len(closing)
                _evict_union(next(iter(_UNIONS)), closing)
                freed += sum(v.nbytes for v in closing[n0:])
            _UNION_BYTES[0] += need
            if self.registry.on_evict.count(_purge_batchers) == 0:
                self.registry.on_evict.append(_purge_batchers)
        _close_unions(closing)
        closing = []
        try:
            v = runion.UnionView(stores)
        except BaseException:
            with _STATE_LOCK:
                _UNION_BYTES[0] -= need
            raise
        v.users, v.evicted = 1, False
        with _STATE_LOCK:
            _UNION_BYTES[0] += v.nbytes - need
            if key in _UNIONS:  # (cannot happen while the caller holds the member locks; stay consistent)
                _evict_union(key, closing)
            _UNIONS[key] = v
        _close_unions(closing)
        return v

    def _run_union_batch(self, names, metadata_filter, items):
        """Batch runner over a store list: one embedding GEMM, one scan + merge of the members'
        union.  Returns per item [(score, member index, row, store)] or None per item when the
        list is not eligible (then the caller takes the per-store path)."""
        stores = [self.registry.get(n) for n in names]
        if any(st is None for st in stores) or not runion.eligible(stores):
            return [None] * len(items)
        locked = sorted(set(stores), key=lambda st: st.name)  # one global order: no lock-order deadlock
        for st in locked:  # members hold their locks while the view is built and searched
            st.lock.acquire()
        view = None
        try:
            view = self._union_view(names, stores)
            if view is None:  # over the view cache's byte budget: the per-store path
                return [None] * len(items)
            mask = view.row_mask(stores, metadata_filter) if metadata_filter is not None else None
            if metadata_filter is not None and mask is None:
                return [[] for _ in items]
            diverse = any(len(it) > 2 for it in items)  # (question, k, (lambda, fetch_k))
            kmax = max(it[1] for it in items)
            with torch.cuda.device(view.device):
                q = self.embedder(view.dim).embed_texts([it[0] for it in items], view.dtype)
                if diverse:  # one selection over the view's rows: diversified across the stores
                    s, r = _search_diverse(view.index, q, items, 2, mask)
                    s, r = s.numpy(), r.numpy()
                else:
                    s, r = view.index.search(q, kmax, row_mask=mask)
                    s, r = s.cpu().numpy(), r.cpu().numpy()
            si, lr = view.locate(r)
            # (the members' locks are held: no compaction renumbers them between the search and here)
            gens = [getattr(st, "generation", None) for st in stores]
            out = []
            for i, it in enumerate(items):
                out.append([(float(s[i, j]), int(si[i, j]), int(lr[i, j]), stores[si[i, j]], gens[si[i, j]])
                            for j in range(it[1]) if r[i, j] >= 0])
            return out
        finally:
            if view is not None:
                _release_union(view)
            for st in reversed(locked):
                st.lock.release()

    def _search_union(self, names, question, k, filt, diversity=None):
        if self.batching:
            key = (tuple(names), filters.filter_key(filt), id(self.registry))
            with _STATE_LOCK:
                b = _BATCHERS.get(key)
                if b is None:
                    b = GroupBatcher(lambda items, n=tuple(names), f=filt: self._run_union_batch(n, f, items),
                                     max_batch=256)
                    if len(_BATCHERS) >= 4096:
                        _BATCHERS.clear()
                    _BATCHERS[key] = b
            return b.submit((question, int(k)) + ((diversity,) if diversity else ()))
        return self._run_union_batch(tuple(names), filt, [(question, int(k)) + ((diversity,) if diversity else ())])[0]

    def search(self, store_names, question, k, metadata_filter=None, diversity=None, hybrid=None, distinct=None):
        """Top-k hits over the union of the named stores, rank order (score desc, store order,
        row asc).  metadata_filter: {key: scalar | [scalars]} over upload metadata (rfx.filters).
        Several flat stores on one device: one scan of their union (rfx.union).
        diversity: None, a lambda in [0, 1], or {"lambda": .., "fetch_k": ..}: the k hits are picked by MMR
        from the fetch_k best (default min(64, max(4k, 16))), in pick order on the union path (diversified
        across the stores); on the per-store path each store's answer is diversified on its own and the
        answers merged by score.  ValueError on a sharded or IVF store.
        hybrid: None, an alpha in [0, 1], or {"alpha", "fetch_k", "rrf_c", "k1", "b"} (parse_hybrid): each store
        answers with the reciprocal-rank fusion of its dense and its BM25 top fetch_k (alpha 1 = dense only),
        Hit.score is the fused score, and several stores are merged by it (never a union view).  ValueError
        (HYBRID_ERROR) on a sharded or IVF store and together with diversity.
        distinct: None, True or {"fetch_k": n} (parse_distinct): the k hits are the best chunks of k DIFFERENT
        files — of the full ranking, a row is kept when no earlier row belongs to the same file (DESIGN §4.17;
        exact over the whole store, not a post-filter of the best rows).  Several stores answer each on its own
        and are merged by score (files of different stores are different documents), never a union view.
        ValueError (DISTINCT_ERROR) on a sharded or IVF store and together with diversity or hybrid."""
        k = int(k)
        if not 1 <= k <= 64:
            raise ValueError(f"top_k={k} out of range [1, 64]")
        filt = filters.check_filter(metadata_filter)
        div = parse_diversity(diversity, k)
        hyb = parse_hybrid(hybrid, k)
        if hyb and div:  # an RRF score is not a similarity: the MMR objective would be meaningless
            raise ValueError(HYBRID_ERROR)
        dst = parse_distinct(distinct, k)
        if dst and (div or hyb):
            raise ValueError(DISTINCT_ERROR)
        self.last_diversity = None
        self.last_hybrid = None
        names = list(dict.fromkeys(store_names or []))
        if self.union and len(names) > 1 and not hyb and not dst:
            res = self._search_union(names, question, k, filt, div)
            if res is not None:
                self.last_path = "union"
                self.last_diversity = "union" if div else None
                hits = []
                for sc, si, row, st, gen in res:
                    info = st.row_info(row, gen)
                    if info is None:
                        continue
                    fid, text, title, uri = info
                    hits.append(Hit(sc, names[si], row, fid, text, title, uri))
                return hits[:k]
        self.last_path = "per-store"
        hits = []
        for si, name in enumerate(names):
            st = self.registry.get(name)
            if st is None or st.index.rows == 0:
                continue
            if div and not _diversity_ok(st):
                raise ValueError(DIVERSITY_ERROR)
            if hyb and not _diversity_ok(st):
                raise ValueError(HYBRID_ERROR)
            if dst and not _distinct_ok(st):
                raise ValueError(DISTINCT_ERROR)
            res = self.search_store(name, question, k, filt, div, hyb, dst) if dst else \
                self.search_store(name, question, k, filt, div, hyb)
            if div:
                self.last_diversity = "store"
            if hyb:
                self.last_hybrid = "store"
            if res is None:
                continue
            st, s, r = res
            gen = getattr(res, "generation", None)
            for sc, row in zip(s, r):
                info = st.row_info(row, gen) if row >= 0 else None
                if info is None:
                    continue
                fid, text, title, uri = info
                hits.append((-sc, si, row, Hit(sc, name, row, fid, text, title, uri)))
        hits.sort(key=lambda h: h[:3])
        return [h[3] for h in hits[:k]]
