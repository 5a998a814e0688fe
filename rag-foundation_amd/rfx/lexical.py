"""Lexical (BM25) index over the hashed term features, and the rank fusion with the dense top-k
(C ABI: rfx_lex_*; rules: DESIGN §4.14, restated by tests/lex_ref.py).

The keyword half of a hybrid answer: the retrieval slice of ask_stream (gemini_rag.py:517-551) ranks by the
dense embedding alone, which smears a part number or an error code over every dimension.  The rows are the CSR
embedder.featurize already produces for the embedder; there is no CPU fallback."""
import ctypes
import threading

import numpy as np
import torch

from . import embedder as _emb
from ._lib import check, lib, ptr, stream_ptr

DEFAULT_K1 = 1.2
DEFAULT_B = 0.75
DEFAULT_RRF_C = 60


def _csr(csr):
    indptr, bucket, count = csr
    indptr = np.ascontiguousarray(indptr, dtype=np.int32)
    bucket = np.ascontiguousarray(bucket, dtype=np.int32)
    count = np.ascontiguousarray(count, dtype=np.int16)
    if indptr.ndim != 1 or indptr.size < 1 or bucket.shape != count.shape or bucket.ndim != 1:
        raise ValueError("a CSR is (indptr [n + 1], bucket [nnz], count [nnz])")
    if indptr.size > 1 and int(indptr.max()) > bucket.size:
        raise ValueError(f"indptr reaches {int(indptr.max())}, the CSR holds {bucket.size} entries")
    return indptr, bucket, count


class LexIndex:
    def __init__(self, V: int = _emb.DEFAULT_V, hash_seed: int = _emb.DEFAULT_HASH_SEED, device: int = 0):
        self.V = int(V)
        self.hash_seed = int(hash_seed)
        self.device = int(device)
        h = ctypes.c_uint64()
        check(lib.rfx_lex_create(self.V, self.device, ctypes.byref(h)), "rfx_lex_create")
        self.handle = h
        self._lock = threading.RLock()  # a search sizes its workspace and runs under one hold: no append between

    def close(self) -> None:
        if getattr(self, "handle", None) is not None:
            lib.rfx_lex_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- content ---------------------------------------------------------------------------------------
    def add_csr(self, indptr, bucket, count) -> int:
        """Append the rows of a host CSR (embedder.featurize's output); returns the first new row."""
        indptr, bucket, count = _csr((indptr, bucket, count))
        with self._lock, torch.cuda.device(self.device):
            first = self.rows
            check(lib.rfx_lex_add(self.handle, indptr.ctypes.data, bucket.ctypes.data, count.ctypes.data,
                                  indptr.size - 1))
        return first

    def add_texts(self, texts) -> int:
        return self.add_csr(*_emb.featurize_texts(list(texts), self.V, self.hash_seed))

    def tombstone(self, rows) -> None:
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
        with torch.cuda.device(self.device):
            check(lib.rfx_lex_tombstone(self.handle, r.ctypes.data, r.size))

    def info(self):
        """(rows, live rows, entries, the sum of the live rows' lengths)"""
        v = [ctypes.c_int64() for _ in range(4)]
        check(lib.rfx_lex_info(self.handle, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    @property
    def rows(self) -> int:
        return self.info()[0]

    @property
    def live_rows(self) -> int:
        return self.info()[1]

    def df(self) -> np.ndarray:
        out = np.zeros(self.V, dtype=np.int64)
        check(lib.rfx_lex_df(self.handle, out.ctypes.data))
        return out

    # ---- search ----------------------------------------------------------------------------------------
    def workspace_bytes(self, nq: int, k: int) -> int:
        b = ctypes.c_size_t()
        check(lib.rfx_lex_search_workspace_bytes(self.handle, int(nq), int(k), ctypes.byref(b)))
        return b.value

    def search(self, csr_or_texts, k: int, k1: float = DEFAULT_K1, b: float = DEFAULT_B, row_mask=None, stream=None,
               out=None, workspace=None):
        """BM25 top-k per question: (scores f32 [nq][k], rows int64 [nq][k]) on the device, padded (-inf, -1).
        Questions: a host CSR (indptr, bucket, count) or a list of strings.  row_mask as DeviceIndex.search.
        out: optional (scores, rows) tensors to write into; workspace: overrides the workspace (tests)."""
        if isinstance(csr_or_texts, (tuple, list)) and len(csr_or_texts) == 3 and \
                not any(isinstance(x, str) for x in csr_or_texts):
            indptr, bucket, count = _csr(csr_or_texts)
        else:
            indptr, bucket, count = _csr(_emb.featurize_texts(list(csr_or_texts), self.V, self.hash_seed))
        nq = indptr.size - 1
        dev = torch.device("cuda", self.device)
        if out is None:
            out_s = torch.empty((nq, max(int(k), 0)), dtype=torch.float32, device=dev)
            out_r = torch.empty((nq, max(int(k), 0)), dtype=torch.int64, device=dev)
        else:
            out_s, out_r = out
        m, mw = None, 0
        if row_mask is not None:
            if row_mask.dtype not in (torch.int32, torch.uint32) or row_mask.dim() != 1 or \
                    not row_mask.is_contiguous() or row_mask.device != dev:
                raise ValueError(f"row mask must be a contiguous 1-D int32/uint32 tensor on {dev}")
            m, mw = row_mask, row_mask.numel()
        with self._lock, torch.cuda.device(dev):
            if workspace is None:
                need = self.workspace_bytes(nq, k) if 1 <= nq <= 1024 and 1 <= k <= 64 else 1
                workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
            check(lib.rfx_lex_search(self.handle, indptr.ctypes.data, bucket.ctypes.data, count.ctypes.data, nq, int(k),
                                     float(k1), float(b), ptr(m) if m is not None else None, mw, ptr(out_s), ptr(out_r),
                                     ptr(workspace), workspace.numel(), stream_ptr(stream)))
        return out_s, out_r

    # ---- fusion ----------------------------------------------------------------------------------------
    def fuse(self, dense_rows: torch.Tensor, lex_rows: torch.Tensor, k: int, alpha, n_dense=None, n_lex=None,
             rrf_c: int = DEFAULT_RRF_C, ranks: bool = False, stream=None, out=None):
        """Reciprocal-rank fusion of two candidate lists per question (rfx_lex_fuse): dense_rows [nq][n_d],
        lex_rows [nq][n_l] int64 as the searches return them (rows < 0 = padding).  alpha: one float or [nq] in
        [0, 1] (1 = dense only); n_dense / n_lex: None, an int or [nq] ints = how many entries of its lists a
        question uses.  Returns (scores f32 [nq][k], rows int64 [nq][k]) and, with ranks, int32 [nq][k][2]."""
        if dense_rows.dim() != 2 or lex_rows.dim() != 2 or dense_rows.shape[0] != lex_rows.shape[0]:
            raise ValueError("the lists must be [nq][n_dense] and [nq][n_lex]")
        dev = torch.device("cuda", self.device)
        if dense_rows.dtype != torch.int64 or lex_rows.dtype != torch.int64 or dense_rows.device != dev or \
                lex_rows.device != dev:
            raise ValueError(f"the lists must be int64 tensors on {dev}")
        dr, lr = dense_rows.contiguous(), lex_rows.contiguous()
        nq = dr.shape[0]
        al = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, dtype=np.float32), (nq,)))
        nd = None if n_dense is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n_dense, dtype=np.int32), (nq,)))
        nl = None if n_lex is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n_lex, dtype=np.int32), (nq,)))
        kk = max(int(k), 0)
        if out is None:
            out_s = torch.empty((nq, kk), dtype=torch.float32, device=dev)
            out_r = torch.empty((nq, kk), dtype=torch.int64, device=dev)
            out_k = torch.empty((nq, kk, 2), dtype=torch.int32, device=dev) if ranks else None
        else:
            out_s, out_r, out_k = out
        with torch.cuda.device(dev):
            check(lib.rfx_lex_fuse(self.handle, ptr(dr), int(dr.shape[1]), ptr(lr), int(lr.shape[1]), nq, int(k),
                                   al.ctypes.data, nd.ctypes.data if nd is not None else None,
                                   nl.ctypes.data if nl is not None else None, int(rrf_c), ptr(out_s), ptr(out_r),
                                   ptr(out_k) if out_k is not None else None, stream_ptr(stream)))
        return (out_s, out_r, out_k) if ranks else (out_s, out_r)
