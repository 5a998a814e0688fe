"""DeviceIndex — one vector-store shard resident in HBM (wrapper over an rfx_index_t handle).

This is the vector store behind a File Search store name (GeminiRag.create_store,
backend/app/services/gemini_rag.py:271-304) and the target of the index write
(upload_file, gemini_rag.py:307-352) and of retrieval (ask_stream, gemini_rag.py:517-551).
Layout in HBM: row-major [capacity][dim] of the index dtype (f32 / bf16 / f16).
"""
import ctypes

import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr


class DeviceIndex:
    def __init__(self, dim: int, dtype: str = "bf16", device: int = 0, capacity: int = 0, _handle=None):
        if dtype not in _lib.DTYPE_CODES:
            raise ValueError(f"dtype must be one of {list(_lib.DTYPE_CODES)}")
        self.dim = int(dim)
        self.dtype = dtype
        self.device = int(device)
        if _handle is not None:
            self.handle = _handle
        else:
            h = ctypes.c_uint64()
            check(lib.rfx_index_create(self.device, self.dim, _lib.DTYPE_CODES[dtype], int(capacity), ctypes.byref(h)))
            self.handle = h.value

    # ---- lifecycle ----------------------------------------------------------------------------
    @classmethod
    def load(cls, path: str, device: int = 0) -> "DeviceIndex":
        h = ctypes.c_uint64()
        check(lib.rfx_index_load(path.encode(), int(device), ctypes.byref(h)))
        dim, dt = ctypes.c_int(), ctypes.c_int()
        check(lib.rfx_index_info(h.value, ctypes.byref(dim), ctypes.byref(dt), None, None, None))
        name = {v: k for k, v in _lib.DTYPE_CODES.items()}[dt.value]
        return cls(dim.value, name, device, _handle=h.value)

    def save(self, path: str) -> None:
        check(lib.rfx_index_save(self.handle, path.encode()))

    def rows_append(self, path: str, row0: int, file_base: int = 0) -> None:
        """Write rows [row0, rows) to the store's append-only row file (fsync'ed); index row i is
        file row file_base + i."""
        with torch.cuda.device(self.device):
            check(lib.rfx_rows_append(self.handle, path.encode(), int(row0), int(file_base)))

    def rows_sync(self, path: str, upto: int, file_base: int = 0) -> None:
        """Append file rows [file_base + rows, file_base + upto) written by another process."""
        with torch.cuda.device(self.device):
            check(lib.rfx_rows_sync(self.handle, path.encode(), int(upto), int(file_base)))

    def data_ptr(self) -> int:
        """Device address of row 0 (rows contiguous, row-major, tombstoned rows NaN).  Valid until
        the next add / reserve / rows_sync, which may reallocate: the owner's lock must be held
        across every use (rfx.store.LocalStore.search)."""
        p = ctypes.c_void_p()
        check(lib.rfx_index_data(self.handle, ctypes.byref(p)))
        return p.value

    def mask_tensor(self, words):
        """Row-mask words (numpy int32) as the device tensor the masked search takes."""
        return torch.from_numpy(words).to(self._dev())

    def close(self) -> None:
        if getattr(self, "handle", None):
            check(lib.rfx_index_destroy(self.handle))
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- info ---------------------------------------------------------------------------------
    def _info(self):
        rows, cap, live = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        check(lib.rfx_index_info(self.handle, None, None, ctypes.byref(rows), ctypes.byref(cap), ctypes.byref(live)))
        return rows.value, cap.value, live.value

    @property
    def rows(self) -> int:
        return self._info()[0]

    @property
    def capacity(self) -> int:
        """Rows the device buffer holds (rows beyond `rows` are NaN); a union view maps members whole."""
        return self._info()[1]

    @property
    def live_rows(self) -> int:
        return self._info()[2]

    @property
    def torch_dtype(self):
        return _lib.TORCH_DTYPES[self.dtype]

    def _dev(self):
        return torch.device("cuda", self.device)

    # ---- writes -------------------------------------------------------------------------------
    def reserve(self, capacity: int) -> None:
        check(lib.rfx_index_reserve(self.handle, int(capacity)))

    def add(self, vecs: torch.Tensor) -> int:
        """Append normalised rows [n][dim] of the index dtype (device or host tensor)."""
        if vecs.dim() != 2 or vecs.shape[1] != self.dim:
            raise ValueError(f"expected [n][{self.dim}] rows, got {tuple(vecs.shape)}")
        if vecs.dtype != self.torch_dtype:
            raise ValueError(f"expected {self.torch_dtype} rows, got {vecs.dtype}")
        vecs = vecs.contiguous()
        first = ctypes.c_int64()
        on_dev = vecs.is_cuda
        st = stream_ptr(torch.cuda.current_stream(vecs.device)) if on_dev else None
        check(lib.rfx_index_add(self.handle, ptr(vecs), vecs.shape[0], int(on_dev), ctypes.byref(first), st))
        return first.value

    def write(self, row0: int, vecs: torch.Tensor) -> None:
        """Overwrite existing rows [row0, row0 + n) with rows of the index dtype (rfx_index_write): they are
        live again and their int8-copy tiles are re-quantised."""
        if vecs.dim() != 2 or vecs.shape[1] != self.dim or vecs.dtype != self.torch_dtype:
            raise ValueError(f"expected [n][{self.dim}] {self.torch_dtype} rows, got {tuple(vecs.shape)} {vecs.dtype}")
        vecs = vecs.contiguous()
        on_dev = vecs.is_cuda
        st = stream_ptr(torch.cuda.current_stream(vecs.device)) if on_dev else None
        check(lib.rfx_index_write(self.handle, int(row0), ptr(vecs), vecs.shape[0], int(on_dev), st))

    def add_synthetic(self, seed: int, n: int, gen_row0: int = -1, stream=None) -> int:
        """Append n generated rows; generator row ids start at gen_row0 (default: continue)."""
        first = ctypes.c_int64()
        with torch.cuda.device(self.device):
            check(lib.rfx_index_add_synthetic(self.handle, ctypes.c_uint64(seed), int(gen_row0), int(n),
                                              ctypes.byref(first), stream_ptr(stream)))
        return first.value

    def tombstone(self, rows) -> None:
        import numpy as np
        arr = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
        with torch.cuda.device(self.device):
            check(lib.rfx_index_tombstone(self.handle, arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), arr.size,
                                          stream_ptr()))

    def compact(self, ranges) -> int:
        """Keep only the rows of `ranges` [(first, count), ...] (ascending, disjoint), gathered in order into
        a fresh, smaller allocation (rfx_index_compact); the int8 copy is rebuilt over them.  Row ids change:
        kept row p is the p-th row of the ranges.  Returns the rows kept.  ValueError for ranges the library
        refuses, before anything moved."""
        arr = _ranges_array(ranges)
        kept = ctypes.c_int64()
        with torch.cuda.device(self.device):
            check(lib.rfx_index_compact(self.handle, arr.ctypes.data if arr.size else None, arr.shape[0],
                                        ctypes.byref(kept), stream_ptr()))
        return kept.value

    def compact_times(self) -> dict:
        """The last compact()'s phases in ms (rfx_index_compact_times): gather = the kernel by HIP events;
        alloc, release, bitmap, screen by the host clock."""
        ms = (ctypes.c_double * 5)()
        check(lib.rfx_index_compact_times(self.handle, ctypes.cast(ms, ctypes.c_void_p)))
        return dict(zip(("gather", "alloc", "release", "bitmap", "screen"), (float(v) for v in ms)))

    def read(self, row0: int, n: int) -> torch.Tensor:
        out = torch.empty((n, self.dim), dtype=self.torch_dtype, device=self._dev())
        with torch.cuda.device(self.device):
            check(lib.rfx_index_read(self.handle, int(row0), int(n), ptr(out), 1, stream_ptr()))
        return out

    # ---- search -------------------------------------------------------------------------------
    def workspace_bytes(self, nq: int, k: int) -> int:
        b = ctypes.c_size_t()
        check(lib.rfx_search_workspace_bytes(self.handle, int(nq), int(k), ctypes.byref(b)))
        return b.value

    def _check_queries(self, q: torch.Tensor):
        if q.dim() != 2 or q.shape[1] != self.dim or q.dtype != self.torch_dtype or not q.is_cuda:
            raise ValueError(f"queries must be a cuda {self.torch_dtype} tensor [nq][{self.dim}]")
        return q.contiguous()

    def _check_mask(self, row_mask, dev):
        """row_mask: None, or a device int32/uint32 bitmap (bit r & 31 of word r >> 5 = row r allowed)
        of at least (rows + 31) // 32 words (make_row_mask)."""
        if row_mask is None:
            return None, 0
        if row_mask.dtype not in (torch.int32, torch.uint32) or row_mask.dim() != 1 or not row_mask.is_contiguous():
            raise ValueError("row mask must be a contiguous 1-D int32/uint32 tensor")
        if row_mask.device != dev:
            raise ValueError(f"row mask on {row_mask.device}, queries on {dev}")
        if row_mask.numel() < (self.rows + 31) // 32:
            raise ValueError(f"row mask has {row_mask.numel()} words, index needs {(self.rows + 31) // 32}")
        return row_mask, row_mask.numel()

    def search(self, queries: torch.Tensor, k: int, workspace: torch.Tensor = None, stream=None,
               row_mask: torch.Tensor = None):
        """Top-k rows per query: (scores f32 [nq][k], rows int64 [nq][k]) on the device.
        row_mask (optional): only rows whose bit is set are returned (metadata filter)."""
        q = self._check_queries(queries)
        nq = q.shape[0]
        dev = q.device
        out_s = torch.empty((nq, k), dtype=torch.float32, device=dev)
        out_r = torch.empty((nq, k), dtype=torch.int64, device=dev)
        need = self.workspace_bytes(nq, k)
        ws = workspace if workspace is not None and workspace.numel() >= need else \
            torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        m, mw = self._check_mask(row_mask, dev)
        with torch.cuda.device(dev):
            if m is None:
                check(lib.rfx_search(self.handle, ptr(q), nq, int(k), ptr(out_s), ptr(out_r), ptr(ws), ws.numel(),
                                     stream_ptr(stream)))
            else:
                check(lib.rfx_search_masked(self.handle, ptr(q), nq, int(k), ptr(m), mw, ptr(out_s), ptr(out_r),
                                            ptr(ws), ws.numel(), stream_ptr(stream)))
        return out_s, out_r

    def search_segmented(self, queries: torch.Tensor, k: int, groups, workspace: torch.Tensor = None, stream=None):
        """One launch for questions under different metadata filters (rfx_search_segmented): `groups` is a
        list of (query_indices, [(first, count), ...]); a query is answered over its group's row ranges only
        (ascending, disjoint, inside the index), and only those rows are read.  Every query belongs to exactly
        one group.  Returns (scores f32 [nq][k], rows int64 [nq][k]) in the caller's query order; a group
        without ranges answers padding (-inf, -1)."""
        q = self._check_queries(queries)
        nq = q.shape[0]
        dev = q.device
        perm, gq, gr, ranges = pack_groups(nq, groups)
        order = torch.as_tensor(perm, dtype=torch.int64, device=dev)
        qs = q.index_select(0, order) if nq else q
        out_s = torch.empty((nq, k), dtype=torch.float32, device=dev)
        out_r = torch.empty((nq, k), dtype=torch.int64, device=dev)
        need = ctypes.c_size_t()
        check(lib.rfx_search_segmented_workspace_bytes(self.handle, nq, int(k), len(ranges) // 2, ctypes.byref(need)))
        ws = workspace if workspace is not None and workspace.numel() >= need.value else \
            torch.empty(max(need.value, 1), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(lib.rfx_search_segmented(self.handle, ptr(qs), nq, int(k), len(gq) - 1, gq.ctypes.data,
                                           gr.ctypes.data, ranges.ctypes.data, ptr(out_s), ptr(out_r), ptr(ws),
                                           ws.numel(), stream_ptr(stream)))
        if nq == 0:
            return out_s, out_r
        inv = torch.empty_like(order)
        inv[order] = torch.arange(nq, dtype=torch.int64, device=dev)
        return out_s.index_select(0, inv), out_r.index_select(0, inv)

    # ---- diversified retrieval (MMR over the top candidates) ----------------------------
    def mmr_workspace_bytes(self, nq: int, n_cand_max: int) -> int:
        b = ctypes.c_size_t()
        check(lib.rfx_mmr_workspace_bytes(self.handle, int(nq), int(n_cand_max), ctypes.byref(b)))
        return b.value

    def mmr_select(self, queries: torch.Tensor, scores: torch.Tensor, rows: torch.Tensor, k: int, lam=0.5,
                   n_cand=None, workspace: torch.Tensor = None, stream=None, return_objective: bool = False):
        """Greedy MMR selection (rfx_mmr_select) of k of each query's candidates: (scores f32, rows int64)
        [nq][n_cand_max] as a search at k = n_cand_max returns them.  lam: one float or [nq] floats in
        [0, 1] (1 = relevance only); n_cand: None, an int, or [nq] ints in 1..n_cand_max = how many of its
        candidates a query uses.  Returns (scores [nq][k], rows [nq][k]) in pick order, padded (-inf, -1),
        and the objectives [nq][k] f32 with return_objective."""
        import numpy as np
        q = self._check_queries(queries)
        nq = q.shape[0]
        dev = q.device
        if scores.shape != rows.shape or scores.dim() != 2 or scores.shape[0] != nq:
            raise ValueError(f"candidates must be [nq={nq}][n_cand] scores and rows of equal shape")
        if scores.dtype != torch.float32 or rows.dtype != torch.int64 or scores.device != dev or rows.device != dev:
            raise ValueError("candidates must be (float32, int64) tensors on the queries' device")
        cs, cr = scores.contiguous(), rows.contiguous()
        n_max = cs.shape[1]
        lam_a = np.ascontiguousarray(np.broadcast_to(np.asarray(lam, dtype=np.float32), (nq,)))
        nc_a = None if n_cand is None else \
            np.ascontiguousarray(np.broadcast_to(np.asarray(n_cand, dtype=np.int32), (nq,)))
        out_s = torch.empty((nq, k), dtype=torch.float32, device=dev)
        out_r = torch.empty((nq, k), dtype=torch.int64, device=dev)
        out_o = torch.empty((nq, k), dtype=torch.float32, device=dev) if return_objective else None
        need = self.mmr_workspace_bytes(nq, n_max)
        ws = workspace if workspace is not None and workspace.numel() >= need else \
            torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(lib.rfx_mmr_select(self.handle, ptr(q), nq, int(n_max), int(k), lam_a.ctypes.data,
                                     nc_a.ctypes.data if nc_a is not None else None, ptr(cs), ptr(cr), ptr(out_s),
                                     ptr(out_r), ptr(out_o) if out_o is not None else None, ptr(ws), ws.numel(),
                                     stream_ptr(stream)))
        return (out_s, out_r, out_o) if return_objective else (out_s, out_r)

    def search_mmr(self, queries: torch.Tensor, k: int, fetch_k: int, lam=0.5, row_mask: torch.Tensor = None):
        """The search at fetch_k, then the MMR selection of k of its answer."""
        if not 1 <= k <= fetch_k <= 64:
            raise ValueError(f"need 1 <= k <= fetch_k <= 64, got k={k} fetch_k={fetch_k}")
        s, r = self.search(queries, int(fetch_k), row_mask=row_mask)
        return self.mmr_select(queries, s, r, int(k), lam=lam)

    # ---- distinct-document search (top-k documents, one best chunk each) --------------------
    def distinct_collapse(self, scores: torch.Tensor, rows: torch.Tensor, k: int, row_doc: torch.Tensor,
                          have: torch.Tensor = None, out=None, stream=None):
        """One collapse of sorted candidate lists by document (rfx_distinct_collapse).  scores f32 / rows int64
        [nq][n_cand] as a search at k = n_cand returns them; row_doc int32 [>= rows] = every row's document
        ordinal, -1 for a row of no live document.  out: None (fresh tensors), or the (scores f32 [nq][k],
        rows int64 [nq][k], docs int32 [nq][k], n int32 [nq], done int32 [nq]) of the round before, which
        with have (int32 [nq], usually out's n) are appended to.  Returns that 5-tuple."""
        if scores.shape != rows.shape or scores.dim() != 2:
            raise ValueError("candidates must be [nq][n_cand] scores and rows of equal shape")
        dev = scores.device
        if scores.dtype != torch.float32 or rows.dtype != torch.int64 or not scores.is_cuda or rows.device != dev:
            raise ValueError("candidates must be (float32, int64) tensors on one device")
        if row_doc.dtype != torch.int32 or row_doc.dim() != 1 or row_doc.device != dev or not row_doc.is_contiguous():
            raise ValueError("row_doc must be a contiguous 1-D int32 tensor on the candidates' device")
        cs, cr = scores.contiguous(), rows.contiguous()
        nq, n_cand = cs.shape
        if out is None:
            out = (torch.empty((nq, k), dtype=torch.float32, device=dev),
                   torch.empty((nq, k), dtype=torch.int64, device=dev),
                   torch.empty((nq, k), dtype=torch.int32, device=dev),
                   torch.empty((nq,), dtype=torch.int32, device=dev),
                   torch.empty((nq,), dtype=torch.int32, device=dev))
        else:
            shapes = ((nq, k), (nq, k), (nq, k), (nq,), (nq,))
            dtypes = (torch.float32, torch.int64, torch.int32, torch.int32, torch.int32)
            if len(out) != 5 or any(t.shape != s or t.dtype != d or t.device != dev or not t.is_contiguous()
                                    for t, s, d in zip(out, shapes, dtypes)):
                raise ValueError(f"out must be contiguous (f32, i64, i32 [{nq}][{k}]; i32, i32 [{nq}]) tensors")
        if have is not None and (have.dtype != torch.int32 or have.shape != (nq,) or have.device != dev
                                 or not have.is_contiguous()):
            raise ValueError(f"have must be a contiguous int32 [{nq}] tensor on the candidates' device")
        with torch.cuda.device(dev):
            check(lib.rfx_distinct_collapse(self.handle, ptr(row_doc), row_doc.numel(), nq, int(n_cand), int(k),
                                            ptr(cs), ptr(cr), ptr(have) if have is not None else None,
                                            ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), ptr(out[4]),
                                            stream_ptr(stream)))
        return out

    def search_distinct(self, queries: torch.Tensor, k: int, row_doc: torch.Tensor, doc_ranges, fetch_k: int = None,
                        row_mask: torch.Tensor = None, select_ranges=None):
        """The exact top-k DOCUMENTS with one best chunk each (rfx.distinct states the rule): the search at
        fetch_k (default default_fetch_k(k); whichever plan `search` takes) and the collapse, then completion
        rounds — ONE segmented search at k = 64 over, per open question, the selected rows without the rows
        of the documents it has found, and a collapse that appends (rfx.distinct.run_rounds).
        row_doc int32 [rows] on the device and doc_ranges [n_docs][2] (first row, rows) describe the documents
        (LocalStore.row_docs); row_mask and select_ranges are the same filter as a bitmap (round 1) and as
        ascending disjoint (first, count) ranges (the completion).  An index whose shape the segmented search
        refuses takes one masked search per open question instead.  Returns (scores f32 [nq][k], rows int64
        [nq][k], docs int32 [nq][k], rounds): device tensors, padded (-inf, -1, -1)."""
        from . import distinct, filters
        k = int(k)
        fetch_k = distinct.default_fetch_k(k) if fetch_k is None else int(fetch_k)
        if not 1 <= k <= fetch_k <= 64:
            raise ValueError(f"need 1 <= k <= fetch_k <= 64, got k={k} fetch_k={fetch_k}")
        q = self._check_queries(queries)
        nq, dev = q.shape[0], q.device
        if not 1 <= nq <= 1024:
            raise ValueError(f"nq={nq} out of [1, 1024]")
        n_rows = self.rows
        if row_doc.numel() == 0:  # an empty index: every candidate is padding, the table is never read
            row_doc = torch.full((1,), -1, dtype=torch.int32, device=dev)
        index = self

        class Ops:
            out = None

            def first(self):
                return index.search(q, fetch_k, row_mask=row_mask)

            def collapse(self, cand, have):
                self.out = index.distinct_collapse(cand[0], cand[1], k, row_doc, self.out[3] if have else None,
                                                   self.out if have else None)

            def read(self):  # one copy to the host: n, done and the docs in one int32 tensor
                host = torch.cat([self.out[3], self.out[4], self.out[2].reshape(-1)]).cpu().numpy()
                return host[:nq], host[nq:2 * nq], host[2 * nq:].reshape(nq, k)

            def _scatter(self, open_q, s, r):
                cs = torch.full((nq, distinct.COMPLETION_K), float("-inf"), dtype=torch.float32, device=dev)
                cr = torch.full((nq, distinct.COMPLETION_K), -1, dtype=torch.int64, device=dev)
                at = torch.as_tensor(open_q, dtype=torch.int64, device=dev)
                cs[at], cr[at] = s, r
                return cs, cr

            def segmented(self, open_q, ranges):
                at = torch.as_tensor(open_q, dtype=torch.int64, device=dev)
                try:
                    s, r = index.search_segmented(q.index_select(0, at), distinct.COMPLETION_K,
                                                  [([i], rg) for i, rg in enumerate(ranges)])
                except _lib.RfxError as e:
                    if e.code == _lib.RFX_EUNSUPPORTED:
                        raise distinct.SegmentedUnsupported(str(e))
                    raise
                return self._scatter(open_q, s, r)

            def masked(self, open_q, ranges):
                res = [index.search(q[i:i + 1], distinct.COMPLETION_K,
                                    row_mask=index.mask_tensor(filters.row_mask_words(n_rows, rg)))
                       for i, rg in zip(open_q, ranges)]
                return self._scatter(open_q, torch.cat([s for s, _ in res]), torch.cat([r for _, r in res]))

        ops = Ops()
        rounds = distinct.run_rounds(ops, nq, k, n_rows, doc_ranges, select_ranges)
        return ops.out[0], ops.out[1], ops.out[2], rounds

    def search_records(self, queries: torch.Tensor, k: int, row_offset: int = 0, out: torch.Tensor = None,
                       workspace: torch.Tensor = None, stream=None, row_mask: torch.Tensor = None) -> torch.Tensor:
        """The search as [nq][k][2] int64 merge records (score bits, row + row_offset): one shard's
        all-gather input (rfx_search_records; the two-pass scan included)."""
        q = self._check_queries(queries)
        nq = q.shape[0]
        if out is None:
            out = torch.empty((nq, k, 2), dtype=torch.int64, device=q.device)
        elif out.shape != (nq, k, 2) or out.dtype != torch.int64 or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous int64 [{nq}][{k}][2] tensor")
        need = self.workspace_bytes(nq, k)
        ws = workspace if workspace is not None and workspace.numel() >= need else \
            torch.empty(max(need, 1), dtype=torch.uint8, device=q.device)
        m, mw = self._check_mask(row_mask, q.device)
        with torch.cuda.device(q.device):
            check(lib.rfx_search_records(self.handle, ptr(q), nq, int(k), ptr(m) if m is not None else None, mw,
                                         int(row_offset), ptr(out), ptr(ws), ws.numel(), stream_ptr(stream)))
        return out

    # ---- the exact two-pass scan (int8 copy of the store) --------------------------------
    def enable_screen(self, mode: int = 1, stream=None) -> None:
        """Keep an int8 copy of the rows (dim bytes per row) and answer searches with the exact
        two-pass scan where it applies (kernel 10: bf16/f16 batches of > 64 questions; kernel 11: up
        to 8 questions of any dtype): int8 screen, exact re-score of the survivors, the exact scan as
        a gated fallback.  mode 0 drops the copy; mode 2 forces the fallback (tests)."""
        with torch.cuda.device(self.device):
            check(lib.rfx_index_screen(self.handle, int(mode), stream_ptr(stream)))

    def screen_state(self):
        """(mode, device bytes of the int8 copy, dropped): dropped = an append outgrew the room the copy
        had (RFX_ECAPACITY) and the library went back to the exact scan."""
        m, b, d = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int()
        check(lib.rfx_index_screen_state(self.handle, ctypes.byref(m), ctypes.byref(b), ctypes.byref(d)))
        return m.value, b.value, bool(d.value)

    def search_plan(self, nq: int, k: int) -> int:
        """Kernel rfx_search runs for (nq, k): 10 = the two-pass scan of a batch (int8 MFMA screen),
        11 = the two-pass scan of up to 8 questions (int8 dot4 screen, one launch)."""
        kern = ctypes.c_int()
        check(lib.rfx_search_plan(self.handle, int(nq), int(k), ctypes.byref(kern)))
        return kern.value

    def screen_read(self, tile0: int, ntiles: int):
        """(codes int8 [ntiles*32][dim], scales f32 [ntiles], live u32 [ntiles], stats f32 [3]: max row norm,
        max quantisation-error norm, max tile scale) of the copy."""
        import numpy as np
        codes = np.empty((ntiles * 32, self.dim), dtype=np.int8)
        scales = np.empty(ntiles, dtype=np.float32)
        live = np.empty(ntiles, dtype=np.uint32)
        stats = np.empty(3, dtype=np.float32)
        with torch.cuda.device(self.device):
            check(lib.rfx_index_screen_read(self.handle, int(tile0), int(ntiles), codes.ctypes.data, scales.ctypes.data,
                                            live.ctypes.data, stats.ctypes.data))
        return codes, scales, live, stats

    def screen_diag(self, nq: int, k: int, workspace: torch.Tensor):
        """After a two-pass search on `workspace`: (diag int32 [nq][2] = kept candidates, survivors
        re-scored (-1: query sent to the fallback); fallback ran for the batch)."""
        import numpy as np
        diag = np.empty((nq, 2), dtype=np.int32)
        fb = ctypes.c_uint32()
        with torch.cuda.device(self.device):
            check(lib.rfx_screen_diag(self.handle, int(nq), int(k), ptr(workspace), diag.ctypes.data, ctypes.byref(fb)))
        return diag, bool(fb.value)

    def screen_valu_diag(self, stream=None) -> bool:
        """After a two-pass search of 1..8 questions (kernel 11) on `stream`: True when the exact fallback
        answered (rfx_screen_valu_diag; read-only)."""
        fb = ctypes.c_uint32()
        with torch.cuda.device(self.device):
            check(lib.rfx_screen_valu_diag(self.handle, stream_ptr(stream), ctypes.byref(fb)))
        return bool(fb.value)

    def list_len(self, nq: int, k: int) -> int:
        """Length of the sorted candidate lists rfx_scan_topk writes (merge hint)."""
        n = ctypes.c_int()
        check(lib.rfx_scan_list_len(self.handle, int(nq), int(k), ctypes.byref(n)))
        return n.value

    def plan(self, nq: int, k: int):
        kern, ncand = ctypes.c_int(), ctypes.c_int64()
        check(lib.rfx_scan_plan(self.handle, int(nq), int(k), ctypes.byref(kern), ctypes.byref(ncand)))
        return kern.value, ncand.value

    def scan(self, queries: torch.Tensor, k: int, workspace: torch.Tensor = None, stream=None,
             row_mask: torch.Tensor = None):
        """Fused scan only: per-query candidate lists (scores f32 [nq][n_cand], local rows int32)."""
        q = self._check_queries(queries)
        nq = q.shape[0]
        _, ncand = self.plan(nq, k)
        cs = torch.empty((nq, ncand), dtype=torch.float32, device=q.device)
        cr = torch.empty((nq, ncand), dtype=torch.int32, device=q.device)
        need = self.workspace_bytes(nq, k)
        ws = workspace if workspace is not None and workspace.numel() >= need else \
            torch.empty(max(need, 1), dtype=torch.uint8, device=q.device)
        m, mw = self._check_mask(row_mask, q.device)
        with torch.cuda.device(q.device):
            if m is None:
                check(lib.rfx_scan_topk(self.handle, ptr(q), nq, int(k), ptr(cs), ptr(cr), ptr(ws), ws.numel(),
                                        stream_ptr(stream)))
            else:
                check(lib.rfx_scan_topk_masked(self.handle, ptr(q), nq, int(k), ptr(m), mw, ptr(cs), ptr(cr),
                                               ptr(ws), ws.numel(), stream_ptr(stream)))
        return cs, cr


SEGMENT_LISTS = 64  # L of the segmented search: a group's rows are cut into at most this many chunks


def pack_groups(nq: int, groups):
    """groups [(query_indices, [(first, count), ...])] -> (perm, group_q, group_r, ranges): the arrays of
    rfx_search_segmented (int64, contiguous); perm[i] = the caller's index of the i-th query in group
    order.  ValueError unless every query index in [0, nq) appears exactly once."""
    import numpy as np
    perm, gq, gr, flat = [], [0], [0], []
    for qidx, rngs in groups:
        perm.extend(int(i) for i in qidx)
        for first, count in rngs:
            flat.extend((int(first), int(count)))
        gq.append(len(perm))
        gr.append(len(flat) // 2)
    if sorted(perm) != list(range(nq)):
        raise ValueError(f"groups must hold each of the {nq} query indices exactly once")
    as64 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.int64))
    return perm, as64(gq), as64(gr), as64(flat if flat else [0, 0])[:len(flat)]


def segmented_plan(rows: int, dim: int, dtype: str, nq: int, k: int, group_q, group_r, ranges):
    """Host only (rfx_segmented_plan): the work list rfx_search_segmented would run over an index of `rows`
    rows, as an int64 array [n_items][4] (group, first query, first selected-row position, selected rows),
    and the candidate lists per query.  ValueError for arguments the search would refuse."""
    import numpy as np
    gq = np.ascontiguousarray(np.asarray(group_q, dtype=np.int64))
    gr = np.ascontiguousarray(np.asarray(group_r, dtype=np.int64))
    rg = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1))
    n_groups = len(gq) - 1
    if n_groups < 0 or len(gr) != len(gq):
        raise ValueError("group_q / group_r must have n_groups + 1 entries each")
    if n_groups and (int(gr[-1]) * 2 > rg.size or int(gr.max()) * 2 > rg.size):
        raise ValueError("group_r points past the ranges")
    n, lists = ctypes.c_int64(), ctypes.c_int()
    args = (int(rows), int(dim), _lib.DTYPE_CODES[dtype], int(nq), int(k), n_groups, gq.ctypes.data, gr.ctypes.data,
            rg.ctypes.data if rg.size else None)
    check(lib.rfx_segmented_plan(*args, None, 0, ctypes.byref(n), ctypes.byref(lists)))
    items = np.empty((n.value, 4), dtype=np.int64)
    check(lib.rfx_segmented_plan(*args, items.ctypes.data if n.value else None, n.value, ctypes.byref(n),
                                 ctypes.byref(lists)))
    return items, lists.value


def _ranges_array(ranges):
    import numpy as np
    arr = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1, 2))
    return arr


def compact_plan(rows: int, ranges):
    """Host only (rfx_compact_plan): what DeviceIndex.compact would do with keep ranges [(first, count), ...]
    over an index of `rows` rows: (kept rows, table int64 [n_ranges][2] = source first row, destination first
    row; chunks int64 [n_chunks][2] = first kept position, positions).  ValueError for ranges the compaction
    refuses."""
    import numpy as np
    arr = _ranges_array(ranges)
    kept, n = ctypes.c_int64(), ctypes.c_int64()
    rp = arr.ctypes.data if arr.size else None
    check(lib.rfx_compact_plan(int(rows), rp, arr.shape[0], None, None, 0, ctypes.byref(kept), ctypes.byref(n)))
    table = np.empty((arr.shape[0], 2), dtype=np.int64)
    chunks = np.empty((n.value, 2), dtype=np.int64)
    check(lib.rfx_compact_plan(int(rows), rp, arr.shape[0], table.ctypes.data if table.size else None,
                               chunks.ctypes.data if chunks.size else None, n.value, ctypes.byref(kept),
                               ctypes.byref(n)))
    return kept.value, table, chunks


def _check_cands(cand_s: torch.Tensor, cand_r: torch.Tensor):
    if cand_s.shape != cand_r.shape or cand_s.dim() != 2:
        raise ValueError("candidate score/row tensors must be [nq][n_cand] of equal shape")
    if cand_r.dtype not in (torch.int32, torch.int64) or cand_s.dtype != torch.float32:
        raise ValueError("candidates must be (float32, int32|int64)")
    return cand_s.contiguous(), cand_r.contiguous()


def topk_merge(cand_s: torch.Tensor, cand_r: torch.Tensor, k: int, row_offset: int = 0, stream=None,
               list_len: int = 1, sorted: bool = False):
    """Merge [nq][n_cand] candidates (rows int32 or int64) into the final top-k per query.
    list_len: the candidates are lists of that length (DeviceIndex.list_len); 1 = no hint.
    sorted: the lists are sorted best first with empty slots at the tail, as DeviceIndex.scan
    writes them (rfx_topk_merge_sorted: a list is read only while it can still contribute)."""
    cand_s, cand_r = _check_cands(cand_s, cand_r)
    nq, ncand = cand_s.shape
    out_s = torch.empty((nq, k), dtype=torch.float32, device=cand_s.device)
    out_r = torch.empty((nq, k), dtype=torch.int64, device=cand_s.device)
    with torch.cuda.device(cand_s.device):
        if sorted:
            check(lib.rfx_topk_merge_sorted(ptr(cand_s), ptr(cand_r), int(cand_r.dtype == torch.int64), nq, ncand,
                                            int(list_len), int(k), int(row_offset), ptr(out_s), ptr(out_r), None,
                                            stream_ptr(stream)))
            return out_s, out_r
        check(lib.rfx_topk_merge_lists(ptr(cand_s), ptr(cand_r), int(cand_r.dtype == torch.int64), nq, ncand,
                                       int(list_len), int(k), int(row_offset), ptr(out_s), ptr(out_r),
                                       stream_ptr(stream)))
    return out_s, out_r


def topk_merge_records(cand_s: torch.Tensor, cand_r: torch.Tensor, k: int, row_offset: int = 0, stream=None,
                       list_len: int = 1, out: torch.Tensor = None, sorted: bool = False) -> torch.Tensor:
    """Merge as topk_merge, writing [nq][k][2] int64 records (score bits, global row): the
    all-gather input of the multi-GPU step (rfx.dist.pack's layout)."""
    cand_s, cand_r = _check_cands(cand_s, cand_r)
    nq, ncand = cand_s.shape
    if out is None:
        out = torch.empty((nq, k, 2), dtype=torch.int64, device=cand_s.device)
    elif out.shape != (nq, k, 2) or out.dtype != torch.int64 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous int64 [{nq}][{k}][2] tensor")
    with torch.cuda.device(cand_s.device):
        if sorted:
            check(lib.rfx_topk_merge_sorted(ptr(cand_s), ptr(cand_r), int(cand_r.dtype == torch.int64), nq, ncand,
                                            int(list_len), int(k), int(row_offset), None, None, ptr(out),
                                            stream_ptr(stream)))
            return out
        check(lib.rfx_topk_merge_records(ptr(cand_s), ptr(cand_r), int(cand_r.dtype == torch.int64), nq, ncand,
                                         int(list_len), int(k), int(row_offset), ptr(out), stream_ptr(stream)))
    return out


def rescore_topk(index: "DeviceIndex", queries: torch.Tensor, scores: torch.Tensor = None, rows: torch.Tensor = None,
                 records: torch.Tensor = None, row_offset: int = 0, stream=None):
    """The score rule of every search (fl32 of the f64 dot; score desc, row asc) applied in place to an
    answer assembled from scan_topk / topk_merge* (rfx_rescore_topk): (scores, rows) [nq][k], or the
    [nq][k][2] records of topk_merge_records (rows carry row_offset).  Returns what it was given."""
    q = index._check_queries(queries)
    nq = q.shape[0]
    if records is not None:
        if records.shape[0] != nq or records.dim() != 3 or records.dtype != torch.int64 or not records.is_contiguous():
            raise ValueError("records must be a contiguous int64 [nq][k][2] tensor")
        k = records.shape[1]
        with torch.cuda.device(q.device):
            check(lib.rfx_rescore_topk(index.handle, ptr(q), nq, int(k), int(row_offset), None, None, ptr(records),
                                       stream_ptr(stream)))
        return records
    if scores.shape != rows.shape or scores.shape[0] != nq or not (scores.is_contiguous() and rows.is_contiguous()):
        raise ValueError("scores / rows must be contiguous [nq][k] tensors")
    with torch.cuda.device(q.device):
        check(lib.rfx_rescore_topk(index.handle, ptr(q), nq, int(scores.shape[1]), int(row_offset), ptr(scores),
                                   ptr(rows), None, stream_ptr(stream)))
    return scores, rows


def merge_gathered(gathered: torch.Tensor, k: int, stream=None):
    """Final merge of all-gathered records [world][nq][k][2] int64 -> (scores [nq][k], rows [nq][k])."""
    if gathered.dim() != 4 or gathered.shape[3] != 2 or gathered.dtype != torch.int64 or gathered.shape[2] != k:
        raise ValueError("gathered must be int64 [world][nq][k][2]")
    g = gathered.contiguous()
    world, nq = g.shape[0], g.shape[1]
    out_s = torch.empty((nq, k), dtype=torch.float32, device=g.device)
    out_r = torch.empty((nq, k), dtype=torch.int64, device=g.device)
    with torch.cuda.device(g.device):
        check(lib.rfx_merge_gathered(ptr(g), int(world), nq, int(k), ptr(out_s), ptr(out_r), stream_ptr(stream)))
    return out_s, out_r


def synth_rows(seed: int, row0: int, n: int, dim: int, dtype: str, device: int = 0) -> torch.Tensor:
    """Synthetic normalised rows generated on the device (same generator as the index)."""
    out = torch.empty((n, dim), dtype=_lib.TORCH_DTYPES[dtype], device=torch.device("cuda", device))
    with torch.cuda.device(device):
        check(lib.rfx_synth_rows(ctypes.c_uint64(seed), int(row0), int(n), int(dim), _lib.DTYPE_CODES[dtype],
                                 ptr(out), stream_ptr()))
    return out
