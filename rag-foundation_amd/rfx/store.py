"""Local File-Search-store equivalent: a DeviceIndex plus per-row chunk metadata, persisted on
disk so that the API processes serve what the ingestion worker wrote (the worker deletes the
uploaded file after indexing, backend/app/services/ingestion.py:341) — SURVEY §8f item 1.

On-disk layout of a store (directory <root>/<store id>/), every data file APPEND-ONLY:
  rows.rfx      rfx_rows_append() row file: 64-byte header + row-major rows (C ABI, include/rfx.h)
  meta.jsonl    one JSON object per row: {"f": file_id, "t": chunk text}
  files.jsonl   file records: {"op": "add", "id", "first", "n", "display_name", "uri", "metadata"}
                and {"op": "del", "id"}
  tombs.bin     int64 row ids of deleted rows
  ivf-<id>.bin  (IVF stores) k-means centroids: "RFXCENT1", u32 nlist, u32 dim, 4 zero bytes,
                then int8 [nlist][dim]; written once per training, never modified
  manifest.json the commit point: {"format": 2, "name", "display_name", "dim", "dtype",
                "generation", "version", "rows", "meta_bytes", "files_bytes", "tombs",
                "index": {"kind": "flat"|"ivf", "nlist", "nprobe", "train_min"},
                "ivf": null | {"id", "rows"}} — the committed length of every file above;
                replaced atomically (rename) after the appended bytes are fsync'ed.  Readers
                never read past it, so a writer that dies mid-append leaves a tail that is
                ignored, and cut by the next writer.
  .lock         fcntl writer lock: appends from several processes (ARQ worker max_jobs=10,
                worker.py:125; several workers) serialise on it, each first catching up with
                what the others committed.
  g-<generation>/  after a compaction (compact()): the directory of the four data files
                above, named by the manifest's "data_dir" (absent: the store directory itself).  A
                compaction writes a whole new generation there (the kept byte ranges of rows.rfx, the
                live rows' metadata, one add record per live file, an empty tombs.bin), commits it
                with one manifest ("compacted": {"from_generation", "from_version", "rows_before",
                "rows", "meta_bytes", "files_bytes"}) and removes the old data files; a g-* directory
                no manifest names is removed by the next writer.
An upload costs O(its own rows) of disk and device work; a reader (API process) that sees a
newer manifest loads only what was appended since its last look (rows, metadata, tombstones).

IVF stores (RFX_INDEX=ivf at creation): the writer trains k-means on the
live rows once there are train_min of them (again at every 8x growth) and commits the centroids
file with the manifest; every process keeps an IvfIndex (rfx.ivf) over the same rows in the same
order, built from the committed centroids and extended incrementally as rows arrive.  Unfiltered
searches probe nprobe lists and re-rank the candidates exactly against the DeviceIndex rows (so
tombstones, NaN there, never return); untrained stores use the exact scan, and so do filtered searches
unless RFX_IVF_FILTERED sends them through the lists under a row mask (search_filtered).

GPU state is a process-level singleton (StoreRegistry), because get_rag_client() builds a new
adapter per request (chat.py:937, ingestion.py:214).
"""
import bisect
import errno
import fcntl
import itertools
import json
import logging
import os
import shutil
import threading
import time
import uuid

import numpy as np

from . import filters
from ._lib import ESIZE, RFX_EBUSY, RfxError, RfxTransientError
from .index import DeviceIndex

log = logging.getLogger("rfx.store")

STORE_PREFIX = "fileSearchStores/"  # accepted by routes/stores.py:46 (prefix check)
FORMAT = 2
_CENT_MAGIC = b"RFXCENT1"
DATA_FILES = ("rows.rfx", "meta.jsonl", "files.jsonl", "tombs.bin")
_ROWS_HDR = 64  # bytes of the row file's header (rfx_rows_append)


def compact_policy():
    """RFX_COMPACT=0 (default: never on its own) | auto: delete_file compacts after its commit when the dead
    rows are at least RFX_COMPACT_MIN_ROWS (default 65,536: the store size from which the project thinks
    extra machinery pays, as RFX_SCREEN_MIN_ROWS) AND at least RFX_COMPACT_MIN_FRACTION of the rows (default
    0.25; DESIGN §4.12 derives it).  Read at every delete: services and tests may change it."""
    mode = os.environ.get("RFX_COMPACT", "0").strip().lower()
    return (mode == "auto", int(os.environ.get("RFX_COMPACT_MIN_ROWS", "65536")),
            float(os.environ.get("RFX_COMPACT_MIN_FRACTION", "0.25")))


def _join_ranges(ranges):
    """(first, count) ranges sorted by first, touching ones joined."""
    out = []
    for first, n in sorted(ranges):
        if out and out[-1][0] + out[-1][1] == first:
            out[-1] = (out[-1][0], out[-1][1] + n)
        else:
            out.append((first, n))
    return out


def _concat(a, b):
    """a followed by b: two device tensors (DeviceIndex.mask_tensor) or two host arrays (host stand-ins)."""
    if isinstance(a, np.ndarray):
        return np.concatenate([a, b])
    import torch
    return torch.cat([a, b])


def _copy_bytes(src_fd, dst_fd, start, n, block=8 << 20):
    """Append bytes [start, start + n) of src to dst (both positioned by the caller for dst)."""
    while n > 0:
        b = os.pread(src_fd, min(n, block), start)
        if not b:
            raise OSError(errno.EIO, f"row file ends before byte {start + n}")
        view = memoryview(b)
        while view:
            view = view[os.write(dst_fd, view):]
        start += len(b)
        n -= len(b)


def _write_file(path, data: bytes):
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC | os.O_CLOEXEC, 0o644)
    try:
        view = memoryview(data)
        while view:
            view = view[os.write(fd, view):]
        os.fsync(fd)
    finally:
        os.close(fd)


def index_spec_from_env():
    """Index kind of new stores: RFX_INDEX=flat (default, exact scan) | ivf (RFX_IVF_NLIST lists,
    default 1024; RFX_IVF_NPROBE, default 32; trained at RFX_IVF_TRAIN_MIN live rows, default
    32 x nlist)."""
    kind = os.environ.get("RFX_INDEX", "flat")
    if kind == "flat":
        return {"kind": "flat"}
    if kind != "ivf":
        raise ValueError(f"RFX_INDEX={kind!r}: expected flat or ivf")
    nlist = int(os.environ.get("RFX_IVF_NLIST", "1024"))
    return {"kind": "ivf", "nlist": nlist, "nprobe": min(int(os.environ.get("RFX_IVF_NPROBE", "32")), nlist, 64),
            "train_min": int(os.environ.get("RFX_IVF_TRAIN_MIN", str(32 * nlist)))}


IVF_MAX_NPROBE = 64  # the C ABI's nprobe limit (rfx_ivf_search)


def ivf_filtered_mode() -> str:
    """RFX_IVF_FILTERED: "0" (default) = a filtered question of an IVF store runs the exact scan, "auto" =
    it takes the posting lists when ivf_filter_nprobe's widened probe count fits the cap, "1" = always, at
    the cap if need be.  Read at every question, as retriever.segmented_mode is."""
    m = os.environ.get("RFX_IVF_FILTERED", "0").strip().lower()
    return m if m in ("auto", "1") else "0"


def ivf_multi_mode() -> bool:
    """RFX_IVF_MULTI: 1 (default) = a batch of filtered questions under different filters takes the posting
    lists in ONE list search (LocalStore.search_lists_filtered_multi); 0 = one list search per
    filter group, as before.  Read at every batch."""
    return os.environ.get("RFX_IVF_MULTI", "1").strip() != "0"


def ivf_filter_nprobe(nprobe, nlist, selected, live, mode):
    """Probe count of a filtered IVF search, or None for the exact path.  A filter that keeps
    `selected` of the `live` rows leaves a fixed nprobe scanning selected / live of the eligible rows an
    unfiltered search scans, and recall falls with it; need = ceil(nprobe * live / selected) keeps the
    expected number of eligible rows scanned at the unfiltered search's.  cap = min(64, nlist).
    mode "auto": need when need <= cap, else None (the exact path's segmented form reads only the selected
    rows); "1": min(need, cap); "0", or selected == 0: None."""
    nprobe, nlist, selected, live = int(nprobe), int(nlist), int(selected), int(live)
    if mode not in ("auto", "1") or selected <= 0:
        return None
    need = -(-nprobe * live // selected)
    cap = min(IVF_MAX_NPROBE, nlist)
    if mode == "1":
        return min(need, cap)
    return need if need <= cap else None


def default_root() -> str:
    return os.environ.get("RFX_INDEX_DIR", os.path.join(os.path.expanduser("~"), ".cache", "rfx", "stores"))


def _fsync_dir(path):
    fd = os.open(path, os.O_RDONLY)
    try:
        os.fsync(fd)
    finally:
        os.close(fd)


def _append(path, committed, data: bytes) -> int:
    """Cut `path` to its committed length (drops a crashed writer's tail), append data, fsync.
    Returns the new committed length."""
    fd = os.open(path, os.O_RDWR | os.O_CREAT | os.O_CLOEXEC, 0o644)
    try:
        os.ftruncate(fd, committed)
        os.lseek(fd, committed, os.SEEK_SET)
        view = memoryview(data)
        while view:
            n = os.write(fd, view)
            view = view[n:]
        os.fsync(fd)
    finally:
        os.close(fd)
    return committed + len(data)


def _read_range(path, start, end) -> bytes:
    if end <= start:
        return b""
    with open(path, "rb") as f:
        f.seek(start)
        b = f.read(end - start)
    if len(b) != end - start:
        raise OSError(errno.EIO, f"{path}: committed range [{start}, {end}) is missing")
    return b


class StoreGone(Exception):
    """The store's manifest no longer exists (dropped by another process)."""


class LocalStore:
    # the vector store behind a LocalStore: DeviceIndex (HIP) in the product; tests inject a host
    # stand-in with the same interface to exercise the file protocol without a GPU
    index_factory = DeviceIndex
    ivf_factory = None  # rfx.ivf.IvfIndex (imported on first use); tests inject a host stand-in

    def __init__(self, path, device, index_factory=None, ivf_factory=None):
        self.path, self.device = path, int(device)
        if index_factory is not None:
            self.index_factory = index_factory
        if ivf_factory is not None:
            self.ivf_factory = ivf_factory
        self.name = self.display_name = None
        self.dim = self.dtype = None
        self.generation = None
        self.index = None
        self.rows = []      # per row: (file_id, chunk text)
        self.files = {}     # file_id -> {"first", "n", "display_name", "uri", "deleted", "metadata"}
        self.version = -1
        self.meta_bytes = self.files_bytes = self.tombs = 0
        self.lock = threading.RLock()
        self._stat = None
        self._masks = {}    # (version, filter key) -> device row mask
        self._ranges = {}   # (version, filter key, form) -> (first, count) row ranges
        self._screen_on = False  # the index holds the two-pass scan's int8 copy (_maybe_screen)
        self.spec = {"kind": "flat"}
        self.ivf_meta = None  # committed {"id", "rows"} of the current centroids
        self.ivf = None       # this process's IvfIndex over the committed rows
        self.ivf_id = None
        self.data_dir = None   # "g-<generation>" after a compaction (manifest "data_dir")
        self.compacted = None  # the manifest's "compacted" record of this generation
        # rows move only in a compaction: _moves is odd while one renumbers this object's rows and even
        # otherwise (numbering()); _prev = the kept ranges of the last one, for hits still in flight
        self._moves = 0
        self._prev = None
        self.on_compact = []  # callbacks(store name) before this object's rows are renumbered
        # the lexical (BM25) index over the chunk texts (rfx.lexical): derived state, built from
        # self.rows by every process (RFX_LEXICAL=1: at open; otherwise at the first lexical() call)
        self._lex = None
        self._lex_dead = set()  # the deleted files whose rows the lexical index has tombstoned
        self._row_docs = None   # row_docs()'s cached answer for one (generation, version)

    # ---- files -------------------------------------------------------------------------------
    def _p(self, name):
        """Path of a store file: the four data files live in the generation's data directory (the store
        directory itself until the first compaction); .lock, the manifest and the centroid files stay put."""
        if self.data_dir and name in DATA_FILES:
            return os.path.join(self.path, self.data_dir, name)
        return os.path.join(self.path, name)

    def _read_manifest(self):
        try:
            with open(self._p("manifest.json"), encoding="utf-8") as f:
                st = os.fstat(f.fileno())
                man = json.load(f)
        except FileNotFoundError:
            return None, None
        if man.get("format") != FORMAT:
            raise RuntimeError(f"{self.path}: store format {man.get('format')} != {FORMAT}")
        return man, (st.st_ino, st.st_mtime_ns, st.st_size)

    def _write_manifest(self, **over):
        """The commit point.  `over`: fields of a state this object has not adopted yet (compact())."""
        man = {"format": FORMAT, "name": self.name, "display_name": self.display_name, "dim": self.dim,
               "dtype": self.dtype, "generation": self.generation, "version": self.version,
               "rows": len(self.rows), "meta_bytes": self.meta_bytes, "files_bytes": self.files_bytes,
               "tombs": self.tombs, "index": self.spec, "ivf": self.ivf_meta}
        if self.data_dir:  # (a store that was never compacted has neither key: its files are where they were)
            man["data_dir"], man["compacted"] = self.data_dir, self.compacted
        man.update(over)
        tmp = self._p(f"manifest.json.{os.getpid()}.{threading.get_ident()}.tmp")
        with open(tmp, "w", encoding="utf-8") as f:
            json.dump(man, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, self._p("manifest.json"))
        _fsync_dir(self.path)
        st = os.stat(self._p("manifest.json"))
        self._stat = (st.st_ino, st.st_mtime_ns, st.st_size)

    class _WriterLock:
        """fcntl lock on <store>/.lock, bounded wait -> RfxTransientError (a TimeoutError: the
        ingestion retry, ingestion.py:35-52, and RETRYABLE_EXCEPTIONS, gemini_rag.py:17-27)."""

        def __init__(self, store):
            self.path = store._p(".lock")
            self.timeout = float(os.environ.get("RFX_LOCK_TIMEOUT_S", "30"))

        def __enter__(self):
            try:
                self.fd = os.open(self.path, os.O_RDWR | os.O_CREAT | os.O_CLOEXEC, 0o644)
            except FileNotFoundError:
                raise StoreGone(self.path)
            t_end = time.monotonic() + self.timeout
            while True:
                try:
                    fcntl.flock(self.fd, fcntl.LOCK_EX | fcntl.LOCK_NB)
                    return self
                except BlockingIOError:
                    if time.monotonic() >= t_end:
                        os.close(self.fd)
                        raise RfxTransientError(RFX_EBUSY, f"store writer lock {self.path} busy "
                                                           f"for {self.timeout:.0f} s")
                    time.sleep(0.005)

        def __exit__(self, *exc):
            fcntl.flock(self.fd, fcntl.LOCK_UN)
            os.close(self.fd)

    # ---- create / open / catch up ---------------------------------------------------------------
    @classmethod
    def create(cls, path, name, display_name, dim, dtype, device, index_factory=None, spec=None,
               ivf_factory=None):
        os.makedirs(path, exist_ok=False)
        st = cls(path, device, index_factory, ivf_factory)
        st.name, st.display_name, st.dim, st.dtype = name, display_name, int(dim), dtype
        st.spec = dict(spec or {"kind": "flat"})
        st.generation = uuid.uuid4().hex
        st.index = st.index_factory(st.dim, dtype, st.device)
        st.version = 0
        with st._WriterLock(st):
            st._write_manifest()
        return st

    @classmethod
    def open(cls, path, device, index_factory=None, ivf_factory=None):
        st = cls(path, device, index_factory, ivf_factory)
        with st.lock:
            st._sync()
        return st

    def _reset(self, man):
        self.name, self.display_name = man["name"], man["display_name"]
        self.dim, self.dtype = int(man["dim"]), man["dtype"]
        self.generation = man["generation"]
        if self.index is not None:
            self.index.close()
        self.index = self.index_factory(self.dim, self.dtype, self.device)
        self.spec = man.get("index") or {"kind": "flat"}
        self.ivf_meta = None
        self._drop_ivf()
        self._drop_lex()
        self.rows, self.files = [], {}
        self.meta_bytes = self.files_bytes = self.tombs = 0
        self.version = -1
        self._masks = {}
        self._ranges = {}
        self._row_docs = None
        self._screen_on = False
        self.data_dir, self.compacted = man.get("data_dir"), man.get("compacted")
        self._prev = None  # (a reload keeps no map from the rows it dropped)

    def _sync(self, man=None, stat=None):
        """Catch up with the committed state on disk (caller holds self.lock).  Incremental: only
        what was appended since the last sync is read.  A compaction by another process removes the
        generation this one may be reading: on an OSError the manifest is read again, and when it names
        another generation the catch-up runs once more against that one."""
        if man is None:
            man, stat = self._read_manifest()
        if man is None:
            raise StoreGone(self.path)
        try:
            return self._sync_to(man, stat)
        except OSError:
            man2, stat2 = self._read_manifest()
            if man2 is None:
                raise StoreGone(self.path)
            if man2["generation"] == man["generation"]:
                raise
            self.generation = None  # whatever was half read belongs to a generation that is gone
        return self._sync_to(man2, stat2)

    def _sync_to(self, man, stat):
        if man["generation"] != self.generation:
            c = man.get("compacted")
            if c and self.index is not None and hasattr(self.index, "compact") \
                    and c["from_generation"] == self.generation and c["from_version"] == self.version \
                    and c["rows_before"] == len(self.rows) and self._follow_compaction(man, c):
                # this object held exactly the state that was compacted: the same ranges, on the device
                if man["version"] == self.version:
                    self.ivf_meta = man.get("ivf")
                    self._ivf_catch_up()
                    self._lex_catch_up()
                    self._maybe_screen()
            else:
                self._reset(man)
        if man["version"] == self.version:
            self._stat = stat
            return
        self.ivf_meta = man.get("ivf")
        n_rows = int(man["rows"])
        if n_rows < len(self.rows) or man["meta_bytes"] < self.meta_bytes or man["files_bytes"] < self.files_bytes \
                or man["tombs"] < self.tombs:
            raise RuntimeError(f"{self.path}: committed state went backwards (same generation)")
        if n_rows > self.index.rows:
            self.index.rows_sync(self._p("rows.rfx"), n_rows)
        for line in _read_range(self._p("meta.jsonl"), self.meta_bytes, man["meta_bytes"]).splitlines():
            o = json.loads(line)
            self.rows.append((o["f"], o["t"]))
        for line in _read_range(self._p("files.jsonl"), self.files_bytes, man["files_bytes"]).splitlines():
            self._apply_file_record(json.loads(line))
        if man["tombs"] > self.tombs:
            raw = _read_range(self._p("tombs.bin"), 8 * self.tombs, 8 * man["tombs"])
            self.index.tombstone(np.frombuffer(raw, dtype="<i8"))
        if len(self.rows) != n_rows or self.index.rows != n_rows:
            raise RuntimeError(f"{self.path}: {len(self.rows)} metadata rows / {self.index.rows} vectors, "
                               f"manifest says {n_rows}")
        self.meta_bytes, self.files_bytes, self.tombs = man["meta_bytes"], man["files_bytes"], man["tombs"]
        self.version = man["version"]
        self._stat = stat
        self._ivf_catch_up()
        self._lex_catch_up()
        self._maybe_screen()

    def _apply_file_record(self, r):
        if r["op"] == "add":
            self.files[r["id"]] = {"first": r["first"], "n": r["n"], "display_name": r["display_name"],
                                   "uri": r["uri"], "deleted": False, "metadata": r.get("metadata")}
        elif r["op"] == "del" and r["id"] in self.files:
            self.files[r["id"]]["deleted"] = True

    def stale(self) -> bool:
        """True when the manifest changed (or vanished) since this process last synced."""
        try:
            st = os.stat(self._p("manifest.json"))
        except FileNotFoundError:
            return True
        return (st.st_ino, st.st_mtime_ns, st.st_size) != self._stat

    def refresh(self) -> bool:
        """Catch up if another process committed; False when the store is gone."""
        with self.lock:
            try:
                self._sync()
            except StoreGone:
                return False
            return True

    # ---- writes (exclusive across processes) ------------------------------------------------------
    def add_document(self, chunks, vecs, display_name, metadata=None):
        with self.lock, self._WriterLock(self):
            self._sync()  # append at the end of what every writer committed
            self._gc_generations()
            file_id = f"files/local-{uuid.uuid4().hex}"
            first = self.index.rows
            # everything after the catch-up is one commit: any failure (ENOSPC, EIO, interrupt) in
            # the row, metadata, file-record or manifest writes re-reads the committed state, so no
            # phantom rows stay in this process's index
            try:
                if len(chunks):
                    self.index.add(vecs)
                    self.index.rows_append(self._p("rows.rfx"), first)
                    meta = "".join(json.dumps({"f": file_id, "t": c}, ensure_ascii=False) + "\n" for c in chunks)
                    self.meta_bytes = _append(self._p("meta.jsonl"), self.meta_bytes, meta.encode())
                rec = {"op": "add", "id": file_id, "first": first, "n": len(chunks), "display_name": display_name,
                       "uri": f"local://{self.name}/{file_id}", "metadata": metadata or None}
                self.files_bytes = _append(self._p("files.jsonl"), self.files_bytes, (json.dumps(rec) + "\n").encode())
                self._apply_file_record(rec)
                self.rows.extend((file_id, c) for c in chunks)
                self._maybe_train()
                self.version += 1
                self._write_manifest()
            except BaseException:
                self._rollback(first)
                raise
            self._ivf_catch_up()
            self._lex_catch_up()
            self._maybe_screen()
            return file_id, first

    def _rollback(self, first):
        """A failed append: drop this process's uncommitted device rows by re-opening from disk."""
        man, stat = self._read_manifest()
        self.generation = None
        self._sync(man, stat)

    # ---- compaction: reclaim the rows of deleted documents ---------------------------------
    def dead_rows(self) -> int:
        """Rows of deleted documents this store still holds (on disk, in device memory, in every scan)."""
        with self.lock:
            return len(self.rows) - sum(f["n"] for f in self.files.values() if not f["deleted"])

    def dead_fraction(self) -> float:
        with self.lock:
            return self.dead_rows() / len(self.rows) if self.rows else 0.0

    def _keep_ranges(self):
        """The live files' row ranges, ascending, touching ones joined: what a compaction keeps."""
        return _join_ranges((f["first"], f["n"]) for f in self.files.values() if not f["deleted"] and f["n"])

    def _gc_generations(self):
        """Writer, under the writer lock, after the catch-up: remove what no manifest names any more — the
        g-* directories of crashed compactions and of generations that were compacted away, and the store
        directory's own data files once a data directory is in force."""
        for name in os.listdir(self.path):
            if name.startswith("g-") and name != self.data_dir:
                shutil.rmtree(os.path.join(self.path, name), ignore_errors=True)
            elif name in DATA_FILES and self.data_dir:
                try:
                    os.unlink(os.path.join(self.path, name))
                except OSError:
                    pass

    def _compacted_state(self, ranges, encode=True):
        """(rows, files, metadata bytes, file-record bytes) of this object's state with only `ranges` kept:
        the live rows' metadata lines and one add record per live file with its new first row.  The writer
        writes the bytes; a reader that follows the compaction on the device adopts the same rows and files
        (encode=False: no bytes; their lengths are in the manifest's "compacted" record)."""
        starts, pos = [], 0
        for first, n in ranges:
            starts.append((first, pos))
            pos += n
        firsts = [s[0] for s in starts]

        def moved(row):  # kept rows before `row` = the new id of a kept row
            i = bisect.bisect_right(firsts, row) - 1
            if i < 0:
                return 0
            return starts[i][1] + min(row - starts[i][0], ranges[i][1])

        rows = [rc for first, n in ranges for rc in self.rows[first:first + n]]
        files, recs = {}, []
        for fid, f in self.files.items():
            if f["deleted"]:
                continue
            rec = {"op": "add", "id": fid, "first": moved(f["first"]), "n": f["n"], "display_name": f["display_name"],
                   "uri": f["uri"], "metadata": f.get("metadata")}
            if encode:
                recs.append(json.dumps(rec) + "\n")
            files[fid] = {"first": rec["first"], "n": f["n"], "display_name": f["display_name"], "uri": f["uri"],
                          "deleted": False, "metadata": f.get("metadata")}
        if not encode:
            return rows, files, None, None
        meta = "".join(json.dumps({"f": fid, "t": t}, ensure_ascii=False) + "\n" for fid, t in rows)
        return rows, files, meta.encode(), "".join(recs).encode()

    def _write_generation(self, data_dir, ranges, meta, recs):
        """The data files of a new generation in <store>/<data_dir>/, each fsync'ed, then the directory.
        rows.rfx = the header and the kept byte ranges of the current row file, copied on the host."""
        d = os.path.join(self.path, data_dir)
        os.mkdir(d)
        if ranges:
            rb = self.dim * ESIZE[self.dtype]
            src = os.open(self._p("rows.rfx"), os.O_RDONLY | os.O_CLOEXEC)
            try:
                dst = os.open(os.path.join(d, "rows.rfx"), os.O_WRONLY | os.O_CREAT | os.O_EXCL | os.O_CLOEXEC, 0o644)
                try:
                    _copy_bytes(src, dst, 0, _ROWS_HDR)
                    for first, n in ranges:
                        _copy_bytes(src, dst, _ROWS_HDR + first * rb, n * rb)
                    os.fsync(dst)
                finally:
                    os.close(dst)
            finally:
                os.close(src)
        _write_file(os.path.join(d, "meta.jsonl"), meta)
        _write_file(os.path.join(d, "files.jsonl"), recs)
        _write_file(os.path.join(d, "tombs.bin"), b"")
        _fsync_dir(d)
        _fsync_dir(self.path)

    def _adopt_compaction(self, ranges, state, generation, version, data_dir, compacted):
        """Renumber this object's rows: the device index keeps `ranges` (no row bytes are read back from
        disk) or, without a compact() (a sharded index, host stand-ins), is reloaded from the new files."""
        rows, files = state[:2]
        for cb in list(self.on_compact):  # union views over this store pin the allocation about to be freed
            cb(self.name)
        self._moves += 1  # odd: searches of this object wait (numbering)
        try:
            # (firsts / pos: each range's first old row and first new row, for row_info's bisect)
            prev = {"generation": self.generation, "ranges": ranges, "firsts": [f for f, _ in ranges],
                    "pos": list(itertools.accumulate((n for _, n in ranges), initial=0))}
            self.generation, self.version = generation, version
            self.data_dir, self.compacted = data_dir, compacted
            self.rows, self.files = rows, files
            self.meta_bytes, self.files_bytes, self.tombs = compacted["meta_bytes"], compacted["files_bytes"], 0
            self._masks, self._ranges = {}, {}
            self._row_docs = None
            if self._screen_on is None:
                self._screen_on = False  # declined for the old generation: this one may fit
            if hasattr(self.index, "compact"):
                kept = self.index.compact(ranges)
                if kept != len(rows):
                    raise RuntimeError(f"{self.path}: the index kept {kept} rows, the store {len(rows)}")
            else:
                self.index.close()
                self.index = self.index_factory(self.dim, self.dtype, self.device)
                self._screen_on = False
                if rows:
                    self.index.rows_sync(self._p("rows.rfx"), len(rows))
            self._prev = prev
            self._drop_ivf()  # the lists hold old row ids; the centroids (ivf_meta, ivf-*.bin) do not
            self._drop_lex()  # old row ids too: rebuilt from the renumbered rows (the same scores: live-row statistics)
        finally:
            self._moves += 1

    def compact(self):
        """Rewrite the store without the rows of deleted documents: a new generation on disk (data files in
        g-<generation>/, one atomic manifest as the commit point), the device rows gathered into a smaller
        allocation.  Row ids change (row_info translates hits of the generation before).  Returns
        {"rows_before", "rows", "seconds"}; nothing is committed when no row is dead."""
        t0 = time.monotonic()
        with self.lock, self._WriterLock(self):
            self._sync()
            self._gc_generations()
            out = self._compact_locked()
        out["seconds"] = time.monotonic() - t0
        return out

    def _compact_locked(self):
        ranges = self._keep_ranges()
        before = len(self.rows)
        kept = sum(n for _, n in ranges)
        if kept == before:
            return {"rows_before": before, "rows": before}
        generation = uuid.uuid4().hex
        data_dir = f"g-{generation}"
        state = self._compacted_state(ranges)
        compacted = {"from_generation": self.generation, "from_version": self.version, "rows_before": before,
                     "rows": kept, "meta_bytes": len(state[2]), "files_bytes": len(state[3])}
        try:  # nothing of this object or of the committed generation is touched before the commit
            self._write_generation(data_dir, ranges, state[2], state[3])
            self._write_manifest(generation=generation, version=self.version + 1, rows=kept, meta_bytes=len(state[2]),
                                 files_bytes=len(state[3]), tombs=0, data_dir=data_dir, compacted=compacted)
        except BaseException:
            try:
                committed = (self._read_manifest()[0] or {}).get("generation") == generation
            except Exception:
                committed = None  # unknown: leave the directory to the next writer's clean-up
            if committed:  # the rename happened and something after it failed: the new generation is in force
                self._rollback(None)
            elif committed is False:
                shutil.rmtree(os.path.join(self.path, data_dir), ignore_errors=True)
            raise
        try:
            self._adopt_compaction(ranges, state, generation, self.version + 1, data_dir, compacted)
        except BaseException:
            self._rollback(None)  # committed: re-open from the new generation's files
            raise
        self._gc_generations()  # the old generation's data files
        self._ivf_catch_up()
        self._lex_catch_up()
        self._maybe_screen()
        return {"rows_before": before, "rows": kept}

    def _follow_compaction(self, man, c):
        """Reader: the manifest's compaction started from exactly this object's state, so the same ranges
        applied to its index give the committed rows; no row bytes are read from disk."""
        ranges = self._keep_ranges()
        state = self._compacted_state(ranges, encode=False)
        if len(state[0]) != c["rows"] or "meta_bytes" not in c or "files_bytes" not in c:
            return False  # not the state the writer had after all: reload
        try:
            self._adopt_compaction(ranges, state, man["generation"], c["from_version"] + 1, man.get("data_dir"), c)
        except BaseException:
            self.generation = None  # the next catch-up reloads
            raise
        return True

    def numbering(self):
        """(token, generation) of this object's row numbering, for code that resolves rows, masks or ranges
        around a search: when numbering_changed(token) is true afterwards, a compaction renumbered the rows
        meanwhile and the work is done again.  Waits while a compaction is moving the rows."""
        while True:
            seq = self._moves
            if seq & 1:
                with self.lock:
                    continue
            return seq, self.generation

    def numbering_changed(self, token) -> bool:
        return self._moves != token

    # ---- IVF (config 5) ------------------------------------------------------------------------------
    def _ivf_enabled(self):
        return self.spec.get("kind") == "ivf" and getattr(self.index, "supports_ivf", True)

    def _new_ivf(self):
        nlist = int(self.spec["nlist"])
        if self.ivf_factory is not None:  # injected (host tests)
            return self.ivf_factory(self.dim, nlist, self.device)
        if hasattr(self.index, "new_ivf"):  # row-sharded store: one list set per shard (rfx.sharded)
            return self.index.new_ivf(nlist)
        from .ivf import IvfIndex
        return IvfIndex(self.dim, nlist, self.device)

    def _drop_ivf(self):
        if self.ivf is not None:
            self.ivf.close()
        self.ivf = self.ivf_id = None

    def _live_rows(self):
        ids = [np.arange(f["first"], f["first"] + f["n"], dtype=np.int64)
               for f in self.files.values() if not f["deleted"] and f["n"]]
        return np.sort(np.concatenate(ids)) if ids else np.zeros(0, dtype=np.int64)

    def _maybe_train(self):
        """Writer, under the writer lock, before the manifest commit: train the coarse quantiser
        when the live rows first reach train_min, and again at every 8x growth since the last
        training; the centroids file is fsync'ed before the manifest that names it."""
        if not self._ivf_enabled():
            return
        live = self._live_rows()
        nlist = int(self.spec["nlist"])
        last = self.ivf_meta["rows"] if self.ivf_meta else 0
        if live.size < max(int(self.spec["train_min"]), nlist) or (last and live.size < 8 * last):
            return
        sample = live[::max(1, live.size // (64 * nlist))]
        ivf = self._new_ivf()
        try:
            ivf.train_from(self.index, sample)
            raw = ivf.centroid_bytes()
        except BaseException:
            ivf.close()
            raise
        cid = uuid.uuid4().hex
        hdr = _CENT_MAGIC + np.array([nlist, self.dim, 0], dtype="<u4").tobytes()
        tmp = self._p(f"ivf-{cid}.bin.tmp")
        with open(tmp, "wb") as f:
            f.write(hdr + raw)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, self._p(f"ivf-{cid}.bin"))
        _fsync_dir(self.path)
        self._drop_ivf()
        self.ivf, self.ivf_id = ivf, cid  # lists are filled by _ivf_catch_up after the commit
        self.ivf_meta = {"id": cid, "rows": int(live.size)}

    def _ivf_catch_up(self):
        """Bring this process's IVF lists up to the committed rows (caller holds self.lock)."""
        if not self._ivf_enabled() or not self.ivf_meta:
            self._drop_ivf()
            return
        cid = self.ivf_meta["id"]
        if self.ivf_id != cid:
            self._drop_ivf()
            with open(self._p(f"ivf-{cid}.bin"), "rb") as f:
                raw = f.read()
            nlist = int(self.spec["nlist"])
            head = np.frombuffer(raw[8:20], dtype="<u4")
            if raw[:8] != _CENT_MAGIC or int(head[0]) != nlist or int(head[1]) != self.dim \
                    or len(raw) != 20 + nlist * self.dim:
                raise RuntimeError(f"{self.path}: centroid file ivf-{cid}.bin is malformed")
            ivf = self._new_ivf()
            ivf.load_centroids(raw[20:])
            self.ivf, self.ivf_id = ivf, cid
        self.ivf.add_from(self.index, self.index.rows)

    # ---- lexical index ------------------------------------------------------------------
    def _drop_lex(self):
        if self._lex is not None:
            self._lex.close()
        self._lex = None
        self._lex_dead = set()

    def _lex_catch_up(self, build=False):
        """Bring this process's lexical index up to the committed rows and deletions (caller holds self.lock):
        the rows appended since (the host featurises their chunk texts) and the rows of the files deleted
        since.  Without an index it does nothing, unless `build` (lexical()) or RFX_LEXICAL=1 ask for one."""
        if self._lex is None:
            if not (build or os.environ.get("RFX_LEXICAL", "0") == "1"):
                return
            from .lexical import LexIndex
            self._lex = LexIndex(device=self.device)
        lex = self._lex
        n = lex.rows
        if n > len(self.rows):  # (cannot happen: a reload or a compaction drops the index)
            self._drop_lex()
            return self._lex_catch_up(build=True)
        for lo in range(n, len(self.rows), 8192):
            lex.add_texts([t for _, t in self.rows[lo:lo + 8192]])
        for fid, f in self.files.items():
            if f["deleted"] and fid not in self._lex_dead:
                if f["n"]:
                    lex.tombstone(np.arange(f["first"], f["first"] + f["n"], dtype=np.int64))
                self._lex_dead.add(fid)

    def lexical(self):
        """The store's lexical index (rfx.lexical.LexIndex), caught up with the committed rows: row r of it is
        row r of the store.  Built on the first call (or at open with RFX_LEXICAL=1); callers search it under
        self.lock, so no append moves it meanwhile."""
        with self.lock:
            self._lex_catch_up(build=True)
            return self._lex

    def _maybe_screen(self):
        """Large stores (d 768 / 1024) answer with the exact two-pass scan: an int8
        copy of the rows (dim bytes per row, kept current by every append / tombstone inside librfx)
        screened on the i8 matrix cores (kernel 10: bf16/f16 batches of > 64 questions) or with
        v_dot4 (kernel 11: up to 8 questions, any dtype), the survivors re-scored exactly.
        RFX_SCREEN=auto (default: from RFX_SCREEN_MIN_ROWS rows, 65,536) | 1 (always) | 0 (never).
        Results are the exact scan's either way.
        The copy is an accelerator, never a condition of a write: this runs after the manifest commit
        (and on every reader's catch-up), so it must not raise.  When the copy does not fit
        (RfxCapacityError: device memory minus a reserve, or RFX_SCREEN_MAX_BYTES) or the build fails,
        the store logs it and stays exact; it is not retried for this store generation (the rows only
        grow).  An append that outgrows the copy later is handled inside librfx the same way (the copy
        is dropped, rfx_index_screen_state)."""
        mode = os.environ.get("RFX_SCREEN", "auto")
        if self._screen_on is True:
            # librfx drops the copy when an append outgrows its room (a sharded index drops every shard's,
            # rfx.sharded): that is a state change of the store, not a detail of one index.
            # The store then answers with the exact plan — the same score rule — and does not retry for
            # this generation, as when the copy was declined up front.
            if hasattr(self.index, "screen_state") and self.index.screen_state()[0] == 0:
                self._screen_on = None
                log.warning("store %s: the int8 copy was dropped by growth; answering with the exact scan",
                            self.name)
            return
        if mode == "0" or self._screen_on is not False or not hasattr(self.index, "enable_screen"):
            return
        if self.dtype not in ("bf16", "f16", "f32") or self.dim not in (768, 1024) or self.index.rows == 0:
            return
        if mode != "1" and self.index.rows < int(os.environ.get("RFX_SCREEN_MIN_ROWS", "65536")):
            return
        try:
            self.index.enable_screen(1)
        except (RfxError, RfxTransientError, ValueError) as e:
            # (transient: the index lock was busy — the next catch-up tries again)
            if not isinstance(e, RfxTransientError):
                self._screen_on = None  # declined for this generation: exact scan
            log.warning("store %s: int8 copy not built (%s); answering with the exact scan", self.name, e)
            return
        self._screen_on = True

    def ivf_ready(self) -> bool:
        return self.ivf is not None and self.ivf.rows == self.index.rows

    def delete_file(self, file_id) -> bool:
        with self.lock, self._WriterLock(self):
            self._sync()
            self._gc_generations()
            f = self.files.get(file_id)
            if not f or f["deleted"]:
                return False
            try:  # one commit, as in add_document: a failure re-reads the committed state
                if f["n"]:
                    rows = np.arange(f["first"], f["first"] + f["n"], dtype="<i8")
                    self.index.tombstone(rows)
                    _append(self._p("tombs.bin"), 8 * self.tombs, rows.tobytes())
                    self.tombs += len(rows)
                rec = {"op": "del", "id": file_id}
                self.files_bytes = _append(self._p("files.jsonl"), self.files_bytes, (json.dumps(rec) + "\n").encode())
                self._apply_file_record(rec)
                self.version += 1
                self._write_manifest()
            except BaseException:
                self._rollback(None)
                raise
            self._lex_catch_up()
            self._auto_compact()
            return True

    def _auto_compact(self):
        """RFX_COMPACT=auto (compact_policy): after a delete's own commit, inside the same writer-lock hold.
        A compaction that fails is logged; the delete has succeeded either way."""
        auto, min_rows, min_fraction = compact_policy()
        if not auto:
            return
        dead = self.dead_rows()
        if dead == 0 or dead < min_rows or dead < min_fraction * len(self.rows):
            return
        try:
            out = self._compact_locked()
            log.info("store %s: compacted %d -> %d rows", self.name, out["rows_before"], out["rows"])
        except Exception as e:
            log.warning("store %s: compaction after a delete failed (%s); the rows stay tombstoned", self.name, e)

    # ---- reads -------------------------------------------------------------------------------------
    def tomb_rows(self, start: int, end: int = None) -> np.ndarray:
        """Committed tombstoned rows [start, end) in commit order (tombs.bin; caller holds self.lock):
        what a follower of this store (rfx.union.UnionView) re-applies after a deletion."""
        end = self.tombs if end is None else end
        if end <= start:
            return np.zeros(0, dtype=np.int64)
        return np.frombuffer(_read_range(self._p("tombs.bin"), 8 * start, 8 * end), dtype="<i8").astype(np.int64)

    def search_gen(self, queries, k):
        """search() plus the generation whose row numbering the answer uses (row_info's argument): a
        compaction that renumbers the rows while the search runs makes it run again.  Unfiltered only: a
        caller that resolves a mask or ranges first brackets that work with numbering() itself."""
        while True:
            token, generation = self.numbering()
            s, r = self.search(queries, k)
            if not self.numbering_changed(token):
                return s, r, generation

    def search(self, queries, k, row_mask=None):
        """(scores, rows) of the top-k rows per query.  An IVF store with trained lists answers
        unfiltered searches from its lists (nprobe probes, exact re-rank of min(64, max(16, 2k))
        candidates); otherwise, and under a metadata filter, the exact scan runs (search_filtered is the
        entry that may take the lists under a filter, RFX_IVF_FILTERED)."""
        if row_mask is None and self.ivf is not None:
            with self.lock:  # the re-rank reads the DeviceIndex rows in place: no append meanwhile
                if self.ivf_ready():
                    s, r = self.ivf.search_index(queries, k, int(self.spec["nprobe"]), self.index,
                                                 rerank_k=min(64, max(16, 2 * int(k))))
                    return s.cpu(), r.cpu()
        return self.index.search(queries, k, row_mask=row_mask)

    def filtered_nprobe(self, metadata_filter):
        """The probe count at which a question under this filter takes the posting lists, or None when it
        takes the exact scan: ivf_filter_nprobe under RFX_IVF_FILTERED over the filter's selected rows
        (the sum of mask_ranges) and the live rows; None too for a flat store or lists that are behind."""
        mode = ivf_filtered_mode()
        if mode == "0" or self.ivf is None:
            return None
        with self.lock:
            if not self.ivf_ready():
                return None
            selected = sum(n for _, n in self.mask_ranges(metadata_filter))
            live = len(self.rows) - self.dead_rows()
            return ivf_filter_nprobe(self.spec["nprobe"], self.spec["nlist"], selected, live, mode)

    def search_lists_filtered(self, queries, k, metadata_filter):
        """The filtered search through the posting lists, or None when the rule (filtered_nprobe) keeps this
        filter on the exact path: (scores, rows) on the host.  The rule, the mask and the search are one
        evaluation under self.lock — as the unfiltered IVF search, the re-rank reads the DeviceIndex rows in
        place."""
        if ivf_filtered_mode() == "0" or self.ivf is None:
            return None
        with self.lock:
            nprobe = self.filtered_nprobe(metadata_filter)
            if nprobe is None:
                return None
            s, r = self.ivf.search_index(queries, k, nprobe, self.index, rerank_k=min(64, max(16, 2 * int(k))),
                                         row_mask=self.row_mask(metadata_filter))
            return s.cpu(), r.cpu()

    def search_lists_filtered_multi(self, queries, k, filters_):
        """One list search for questions under different filters.  filters_: one metadata filter
        per question; equal filters share a mask.  The rule (filtered_nprobe) is evaluated once per distinct
        filter and, with the masks and the search, is one evaluation under self.lock.  The questions whose
        filter the rule sends to the lists are answered together — each at its own filter's probe count under
        its own mask, re-ranked at the depth for k as search_lists_filtered does — in one call of
        search_index.  -> (scores [nq][k], rows [nq][k], declined): host tensors, and the indices of the
        questions the rule keeps exact (their lines are padding, (-inf, -1)); None when nothing takes the
        lists (mode 0, a flat store, every filter declined)."""
        import torch
        nq = len(filters_)
        if queries.shape[0] != nq:
            raise ValueError(f"{queries.shape[0]} questions, {nq} filters")
        if ivf_filtered_mode() == "0" or self.ivf is None:
            return None
        with self.lock:
            table, mask_of, nprobes, slot = [], [-1] * nq, [0] * nq, {}
            for filt, idxs in filters.group_by_filter(list(filters_)):
                nprobe = self.filtered_nprobe(filt)
                mask = self.row_mask(filt) if nprobe is not None else None
                if mask is None:
                    continue
                key = id(mask)
                if key not in slot:
                    slot[key] = len(table)
                    table.append(mask)
                for i in idxs:
                    mask_of[i], nprobes[i] = slot[key], nprobe
            take = [i for i in range(nq) if nprobes[i]]  # in filter-group order: a staged batch of the list scan
            take.sort(key=lambda i: mask_of[i])          # then mostly holds one mask (k_ivf.hip list_scan_multi_kernel)
            if not take:
                return None
            out_s = torch.full((nq, k), float("-inf"), dtype=torch.float32)
            out_r = torch.full((nq, k), -1, dtype=torch.int64)
            q = queries if len(take) == nq and take == list(range(nq)) else queries[take]
            s, r = self.ivf.search_index(q, k, max(nprobes), self.index, rerank_k=min(64, max(16, 2 * int(k))),
                                         row_masks=table, mask_of=[mask_of[i] for i in take],
                                         nprobes=[nprobes[i] for i in take])
            out_s[take], out_r[take] = s.cpu(), r.cpu()
            return out_s, out_r, [i for i in range(nq) if not nprobes[i]]

    def search_filtered(self, queries, k, metadata_filter):
        """(scores, rows, path) of the top-k rows per query among the rows the filter selects, scores and rows
        always on the host.  path "ivf": the posting lists at filtered_nprobe's widened probe count, the row
        mask applied inside the list scan, exact re-rank of min(64, max(16, 2k)) candidates (DESIGN §4.15;
        RFX_IVF_FILTERED=auto|1).  path "exact": the masked exact scan — the default, a probe count past the
        cap under auto, lists that are behind, a flat store.  A filter that matches no file answers padding
        (-inf, -1)."""
        import torch
        mask = self.row_mask(metadata_filter)
        if mask is None:
            nq = queries.shape[0]
            return (torch.full((nq, k), float("-inf"), dtype=torch.float32),
                    torch.full((nq, k), -1, dtype=torch.int64), "exact")
        out = self.search_lists_filtered(queries, k, metadata_filter)
        if out is not None:
            return out[0], out[1], "ivf"
        s, r = self.index.search(queries, k, row_mask=mask)
        return s.cpu(), r.cpu(), "exact"

    def row_mask(self, metadata_filter):
        """Device row mask (int32 words) of the live files whose upload metadata matches the
        filter (rfx.filters), or None when no file matches.  Cached per (store version, filter)."""
        with self.lock:
            key = (self.version, filters.filter_key(metadata_filter))
            if key in self._masks:
                return self._masks[key]
            ranges = self.mask_ranges(metadata_filter)
            mask = None
            if ranges:
                words = filters.row_mask_words(self.index.rows, ranges)
                mask = self.index.mask_tensor(words)
            if len(self._masks) >= 64:
                self._masks.clear()
            self._masks[key] = mask
            return mask

    def mask_ranges(self, metadata_filter):
        """(first, count) row ranges of the live files whose upload metadata matches the filter, in file
        order.  Cached per (store version, filter), as row_mask; callers do not change the list."""
        with self.lock:
            key = (self.version, filters.filter_key(metadata_filter), "files")
            if key not in self._ranges:
                if len(self._ranges) >= 256:
                    self._ranges.clear()
                self._ranges[key] = [(f["first"], f["n"]) for f in self.files.values()
                                     if not f["deleted"] and f["n"] and
                                     filters.file_matches(filters.normalize_metadata(f.get("metadata")), metadata_filter)]
            return self._ranges[key]

    def segment_ranges(self, metadata_filter):
        """mask_ranges in ascending row order with touching ranges joined (files own disjoint row ranges):
        the form the segmented search takes (DeviceIndex.search_segmented).  Cached the same way."""
        with self.lock:
            key = (self.version, filters.filter_key(metadata_filter), "sorted")
            if key not in self._ranges:
                out = []
                for first, n in sorted(self.mask_ranges(metadata_filter)):
                    if out and out[-1][0] + out[-1][1] == first:
                        out[-1] = (out[-1][0], out[-1][1] + n)
                    else:
                        out.append((first, n))
                if len(self._ranges) >= 256:
                    self._ranges.clear()
                self._ranges[key] = out
            return self._ranges[key]

    def row_docs(self):
        """(row_doc, doc_ranges, file_ids) of the current row numbering, for the distinct-document search
        (DeviceIndex.search_distinct): row_doc = the device int32 tensor [rows] of every row's
        document ordinal, -1 for the rows of deleted files; doc_ranges int64 [n_docs][2] = (first row, rows) of
        every ordinal; file_ids[ordinal] = the file id.  An ordinal is a file's position in self.files.
        Cached per (generation, version): after appends alone (the same generation, no new delete) the cached
        copy is extended by the new rows only; a delete or a compaction rebuilds it.  Another process's
        commits arrive through _sync like everything else: callers hold a store they got from the registry."""
        with self.lock:
            c = self._row_docs
            if c is not None and c["key"] == (self.generation, self.version):
                return c["row_doc"], c["doc_ranges"], c["file_ids"]
            n_rows, n_files = len(self.rows), len(self.files)
            dead = sum(1 for f in self.files.values() if f["deleted"])
            grown = c is not None and c["generation"] == self.generation and c["dead"] == dead \
                and c["rows"] <= n_rows and len(c["file_ids"]) <= n_files
            row0, doc0 = (c["rows"], len(c["file_ids"])) if grown else (0, 0)
            fresh = np.full(n_rows - row0, -1, dtype=np.int32)
            for d, f in enumerate(itertools.islice(self.files.values(), doc0, None), doc0):
                if not f["deleted"] and f["n"]:
                    fresh[f["first"] - row0:f["first"] - row0 + f["n"]] = d
            piece = self.index.mask_tensor(fresh)
            row_doc = _concat(c["row_doc"], piece) if grown and row0 else piece
            ranges = np.array([(f["first"], f["n"]) for f in self.files.values()], dtype=np.int64).reshape(-1, 2)
            self._row_docs = {"key": (self.generation, self.version), "generation": self.generation, "dead": dead,
                              "rows": n_rows, "row_doc": row_doc, "doc_ranges": ranges, "file_ids": list(self.files),
                              "extended": bool(grown and row0)}
            return row_doc, ranges, self._row_docs["file_ids"]

    def row_info(self, row, generation=None):
        """(file_id, chunk text, title, uri) of a row, or None for a row this process has no
        metadata for (cannot happen after a consistent sync; guarded anyway).  generation: the one the
        search that returned `row` ran under (numbering / search_gen; None = the current one).  A row of the
        generation just before the last compaction is translated through its kept ranges (None when it was
        deleted); rows of any older generation are unknown: None."""
        while True:  # one numbering throughout: a compaction swaps generation, _prev, rows and files one by one
            token, current = self.numbering()
            out = self._row_info(row, generation, current)
            if not self.numbering_changed(token):
                return out

    def _row_info(self, row, generation, current):
        if generation is not None and generation != current:
            prev = self._prev
            if prev is None or prev["generation"] != generation or row < 0:
                return None
            i = bisect.bisect_right(prev["firsts"], row) - 1
            if i < 0 or row >= prev["firsts"][i] + prev["ranges"][i][1]:
                return None
            row = prev["pos"][i] + row - prev["firsts"][i]
        if not 0 <= row < len(self.rows):
            return None
        fid, text = self.rows[row]
        f = self.files.get(fid, {})
        return fid, text, f.get("display_name"), f.get("uri")

    def close(self):
        with self.lock:
            self._drop_ivf()
            self._drop_lex()
            if self.index is not None:
                self.index.close()


class StoreRegistry:
    """Process-wide map store name -> LocalStore: lazy open, incremental catch-up when another
    process committed, eviction when another process dropped the store."""

    def __init__(self, root=None, device=None, index_factory=None, devices=None, ivf_factory=None):
        """devices (or RFX_DEVICES, e.g. "0,1,2,3,4,5,6,7"; "0x4" = 4 logical shards on device 0):
        more than one -> every store is row-sharded over them (rfx.sharded.ShardedIndex)."""
        self.root = root or default_root()
        self.index_factory = index_factory
        self.device = int(os.environ.get("RFX_DEVICE", "0")) if device is None else int(device)
        spec = devices if devices is not None else os.environ.get("RFX_DEVICES")
        if index_factory is None and spec:
            from .sharded import ShardedIndex, parse_devices
            devs = parse_devices(spec) if isinstance(spec, str) else [int(d) for d in spec]
            if len(devs) > 1:
                self.device = devs[0]
                self.index_factory = lambda dim, dtype, device, _d=tuple(devs): ShardedIndex(dim, dtype, list(_d))
        self.ivf_factory = ivf_factory
        self._stores = {}
        self._lock = threading.Lock()
        self.on_evict = []  # callbacks(name) when a store leaves this registry (rfx.retriever)

    def _dir(self, name):
        if not isinstance(name, str) or not name.startswith(STORE_PREFIX + "local-"):
            return None
        return os.path.join(self.root, name[len(STORE_PREFIX + "local-"):])

    def create(self, display_name, dim, dtype, spec=None):
        """spec: the store's index kind (index_spec_from_env() when None)."""
        name = f"{STORE_PREFIX}local-{uuid.uuid4().hex}"
        os.makedirs(self.root, exist_ok=True)
        st = LocalStore.create(self._dir(name), name, display_name, dim, dtype, self.device, self.index_factory,
                               spec if spec is not None else index_spec_from_env(), self.ivf_factory)
        st.on_compact.append(self._compacted)
        with self._lock:
            self._stores[name] = st
        return st

    def _compacted(self, name):
        """A store of this registry is about to renumber its rows: what was built over the old numbering
        (batchers' cached masks aside, the union views that pin its allocation) goes, as on eviction."""
        for cb in self.on_evict:
            cb(name)

    def _evict(self, name):
        st = self._stores.pop(name, None)
        if st is not None:
            st.close()
        for cb in self.on_evict:
            cb(name)

    def get(self, name):
        with self._lock:
            st = self._stores.get(name)
            if st is not None:
                if not st.stale():
                    return st
                if st.refresh():
                    return st
                self._evict(name)  # dropped by another process (cleanup.py delete_store)
                return None
            d = self._dir(name)
            if d is None or not os.path.exists(os.path.join(d, "manifest.json")):
                return None
            try:
                st = LocalStore.open(d, self.device, self.index_factory, self.ivf_factory)
            except StoreGone:
                return None
            st.on_compact.append(self._compacted)
            self._stores[name] = st
            return st

    def drop(self, name) -> bool:
        with self._lock:
            had = name in self._stores
            self._evict(name)
            d = self._dir(name)
            if d and os.path.isdir(d):
                # the manifest goes first: other processes see the store gone, not half-deleted
                try:
                    os.unlink(os.path.join(d, "manifest.json"))
                except FileNotFoundError:
                    pass
                shutil.rmtree(d, ignore_errors=True)
                return True
            return had

    def names(self):
        out = set(self._stores)
        if os.path.isdir(self.root):
            for d in os.listdir(self.root):
                if os.path.exists(os.path.join(self.root, d, "manifest.json")):
                    out.add(f"{STORE_PREFIX}local-{d}")
        return sorted(out)


_REGISTRY = None
_REG_LOCK = threading.Lock()


def registry() -> StoreRegistry:
    global _REGISTRY
    with _REG_LOCK:
        if _REGISTRY is None:
            _REGISTRY = StoreRegistry()
        return _REGISTRY


def set_registry(reg: StoreRegistry) -> None:
    global _REGISTRY
    with _REG_LOCK:
        _REGISTRY = reg
