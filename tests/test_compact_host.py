"""CPU: the host half of store compaction.  The library exports and declares the new entry
points; rfx_compact_plan, a pure host function, maps every kept position to its source row, tiles the kept
positions exactly once in a bounded number of chunks and refuses every malformed input; LocalStore.compact()
writes a new generation (data files in g-<generation>/, one atomic manifest), survives a failure at every
step before the commit, is followed by other LocalStore objects on the index (no row bytes from disk) or by a
reload; row_info translates hits of the generation before; RFX_COMPACT=auto triggers at its two thresholds."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from fakes import HostIndex
from rfx import store as rstore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rfx.h")
NEW = ("rfx_index_compact", "rfx_compact_plan", "rfx_index_compact_times")
MAX_CHUNKS = 4096


def test_symbols_exported_declared_and_bound():
    from rfx import _lib, index
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rfx_\w+)", out))
    declared = set(re.findall(r"^\s*(?:const char\*|int)\s+(rfx_\w+)\s*\(", open(HEADER).read(), re.M))
    for s in NEW:
        assert s in exported and s in declared and s in _lib.SIGNATURES, s
    assert callable(index.DeviceIndex.compact) and callable(index.compact_plan)


# ---- rfx_compact_plan ---------------------------------------------------------------------------------------
def check_plan(rows, ranges):
    from rfx.index import compact_plan
    kept, table, chunks = compact_plan(rows, ranges)
    want = np.concatenate([np.arange(f, f + n) for f, n in ranges]) if ranges else np.zeros(0, dtype=np.int64)
    assert kept == want.size
    assert table.shape == (len(ranges), 2)
    if ranges:
        assert table[:, 0].tolist() == [f for f, _ in ranges]
        assert table[:, 1].tolist() == np.concatenate([[0], np.cumsum([n for _, n in ranges])[:-1]]).tolist()
    assert len(chunks) <= MAX_CHUNKS and (len(chunks) == 0) == (kept == 0)
    # the chunks tile [0, kept) exactly once, in order
    if kept:
        assert chunks[0, 0] == 0 and (chunks[:, 1] > 0).all()
        assert (chunks[1:, 0] == chunks[:-1, 0] + chunks[:-1, 1]).all()
        assert chunks[-1, 0] + chunks[-1, 1] == kept
        # every destination row maps to the right source row through the table
        p = np.arange(kept)
        i = np.searchsorted(table[:, 1], p, side="right") - 1
        assert np.array_equal(table[i, 0] + (p - table[i, 1]), want)
    return kept, table, chunks


def test_plan_hand_made():
    check_plan(5000, [(0, 1), (3, 1), (20, 12), (32, 40), (100, 60), (300, 3), (304, 3), (308, 3), (4990, 10)])
    check_plan(129, [(31, 1), (32, 1), (127, 2)])        # rows at the 32- and 128-row boundaries
    check_plan(256, [(0, 32), (96, 32), (128, 128)])     # ranges ending / starting on them
    check_plan(7, [(i, 1) for i in range(0, 7, 2)])      # ranges of 1 row
    kept, _, chunks = check_plan(5000, [(0, 5000)])      # keep-all
    assert kept == 5000
    kept, _, chunks = check_plan(5000, [])               # keep-none
    assert kept == 0 and len(chunks) == 0
    check_plan(0, [])


def test_plan_chunks_bounded_independently_of_ranges():
    ranges = [(2 * i, 1) for i in range(300_000)]
    kept, _, chunks = check_plan(600_000, ranges)
    assert kept == 300_000 and len(chunks) <= MAX_CHUNKS
    assert chunks[:, 1].max() > 1  # chunks span ranges


def test_plan_random():
    rng = np.random.default_rng(11)
    for trial in range(60):
        rows = int(rng.integers(1, 60000))
        span = int(rng.integers(1, 40 if trial % 3 else 4000))
        ranges, at = [], 0
        while True:
            first, count = at + int(rng.integers(0, span)), 1 + int(rng.integers(0, span))
            if first >= rows or count > rows - first:
                break
            ranges.append((first, count))
            at = first + count
        check_plan(rows, ranges)


@pytest.mark.parametrize("rows,ranges", [
    (100, [(50, 5), (10, 5)]),      # unsorted
    (100, [(10, 5), (14, 5)]),      # overlapping
    (100, [(96, 5)]),               # past the end
    (100, [(100, 1)]),
    (100, [(-1, 5)]),
    (100, [(10, 0)]),               # empty
    (100, [(10, -2)]),
    (100, [(10, 2 ** 62)]),
    (0, [(0, 1)]),
    (-1, []),
    (2 ** 31, []),
])
def test_plan_refuses_malformed(rows, ranges):
    from rfx.index import compact_plan
    with pytest.raises(ValueError):
        compact_plan(rows, ranges)


# ---- the file protocol, with host stand-ins ---------------------------------------------------------------------
class PlainIndex(HostIndex):
    """A stand-in without compact(): the store reloads it from the new generation's files."""


class CompactingIndex(HostIndex):
    """A stand-in with compact(): the store keeps its rows in place (no row bytes from disk)."""
    calls = []

    def compact(self, ranges):
        CompactingIndex.calls.append(list(ranges))
        keep = np.concatenate([np.arange(f, f + n) for f, n in ranges]) if ranges else np.zeros(0, dtype=np.int64)
        self.data = self.data[keep]
        return int(keep.size)


def reg(root, factory):
    return rstore.StoreRegistry(root=str(root), device=0, index_factory=factory)


def vecs(n, seed, dim=64):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


def build(root, factory):
    """Five documents (one of them empty), two deleted: rows 0-2 A, 3-4 B (deleted), 5-8 C, 9 D (deleted), 10-11 E."""
    r = reg(root, factory)
    st = r.create("demo", 64, "f32")
    ids = {}
    for name, n, seed in (("A", 3, 1), ("B", 2, 2), ("C", 4, 3), ("D", 1, 4), ("E", 2, 5)):
        ids[name] = st.add_document([f"{name}{i}" for i in range(n)], vecs(n, seed), f"{name}.md", {"doc": name})[0]
    ids["Z"] = st.add_document([], vecs(0, 6), "Z.md")[0]
    st.delete_file(ids["B"])
    st.delete_file(ids["D"])
    return r, st, ids


KEPT_TEXT = ["A0", "A1", "A2", "C0", "C1", "C2", "C3", "E0", "E1"]
KEPT_ROWS = [0, 1, 2, 5, 6, 7, 8, 10, 11]


def data_files(path):
    return sorted(n for n in os.listdir(path) if n in rstore.DATA_FILES)


@pytest.mark.parametrize("factory", [PlainIndex, CompactingIndex])
def test_compact_writes_a_new_generation(tmp_path, factory):
    CompactingIndex.calls.clear()
    r, st, ids = build(tmp_path, factory)
    old_rows = open(st._p("rows.rfx"), "rb").read()
    old_data = st.index.data.copy()
    gen0, ver0 = st.generation, st.version
    assert st.dead_rows() == 3 and st.dead_fraction() == pytest.approx(3 / 12)
    out = st.compact()
    assert out["rows_before"] == 12 and out["rows"] == 9 and out["seconds"] >= 0
    assert st.dead_rows() == 0 and st.generation != gen0 and st.version == ver0 + 1
    if factory is CompactingIndex:
        assert CompactingIndex.calls == [[(0, 3), (5, 4), (10, 2)]]
    man = json.load(open(os.path.join(st.path, "manifest.json")))
    assert man["format"] == 2 and man["data_dir"] == f"g-{man['generation']}" and man["rows"] == 9 and man["tombs"] == 0
    assert {k: man["compacted"][k] for k in ("from_generation", "from_version", "rows_before", "rows")} == \
        {"from_generation": gen0, "from_version": ver0, "rows_before": 12, "rows": 9}
    # the data files moved to the generation's directory; the old ones are gone; the rest stayed
    d = os.path.join(st.path, man["data_dir"])
    assert data_files(st.path) == [] and data_files(d) == sorted(rstore.DATA_FILES)
    assert os.path.exists(os.path.join(st.path, ".lock"))
    rb = 64 * 4
    want = old_rows[:64] + b"".join(old_rows[64 + f * rb:64 + (f + n) * rb] for f, n in [(0, 3), (5, 4), (10, 2)])
    assert open(os.path.join(d, "rows.rfx"), "rb").read() == want
    assert os.path.getsize(os.path.join(d, "tombs.bin")) == 0
    recs = [json.loads(x) for x in open(os.path.join(d, "files.jsonl"))]
    assert [(x["op"], x["id"], x["first"], x["n"]) for x in recs] == \
        [("add", ids["A"], 0, 3), ("add", ids["C"], 3, 4), ("add", ids["E"], 7, 2), ("add", ids["Z"], 9, 0)]
    # this object and a fresh open see exactly the live files' chunks, in order
    fresh = reg(tmp_path, factory).get(st.name)
    for s in (st, fresh):
        assert [t for _, t in s.rows] == KEPT_TEXT and s.index.rows == 9
        assert np.array_equal(s.index.data, old_data[KEPT_ROWS])
        assert {f: (v["first"], v["n"]) for f, v in s.files.items()} == \
            {ids["A"]: (0, 3), ids["C"]: (3, 4), ids["E"]: (7, 2), ids["Z"]: (9, 0)}
        assert s.files[ids["C"]]["metadata"] == {"doc": "C"} and s.row_info(3)[:3] == (ids["C"], "C0", "C.md")
    # the new generation takes appends and deletes like any other
    f6, first = st.add_document(["F0"], vecs(1, 7), "F.md")
    assert first == 9
    st.delete_file(ids["A"])
    fresh.refresh()
    assert [t for _, t in fresh.rows] == KEPT_TEXT + ["F0"] and fresh.files[ids["A"]]["deleted"]
    assert np.isnan(fresh.index.data[:3]).all() and not np.isnan(fresh.index.data[3:]).any()


def test_compact_without_dead_rows_commits_nothing(tmp_path):
    r = reg(tmp_path, CompactingIndex)
    st = r.create("demo", 64, "f32")
    st.add_document(["a", "b"], vecs(2, 1), "a.md")
    before = open(os.path.join(st.path, "manifest.json")).read()
    out = st.compact()
    assert out["rows_before"] == out["rows"] == 2
    assert open(os.path.join(st.path, "manifest.json")).read() == before
    assert "data_dir" not in json.loads(before)  # a store that was never compacted has no data_dir ...
    assert reg(tmp_path, CompactingIndex).get(st.name).index.rows == 2  # ... and opens as before
    assert not [n for n in os.listdir(st.path) if n.startswith("g-")]


def test_compact_everything_deleted(tmp_path):
    r, st, ids = build(tmp_path, CompactingIndex)
    for k in "ACEZ":
        st.delete_file(ids[k])
    assert st.compact()["rows"] == 0
    assert st.index.rows == 0 and st.rows == [] and st.files == {}
    assert reg(tmp_path, CompactingIndex).get(st.name).index.rows == 0
    _, first = st.add_document(["n0", "n1"], vecs(2, 9), "n.md")
    assert first == 0 and reg(tmp_path, CompactingIndex).get(st.name).index.rows == 2


class Boom(Exception):
    pass


def _fail_nth(monkeypatch, target, name, nth):
    """Make the nth call (1-based) of target.name raise Boom; earlier calls pass through."""
    real, seen = getattr(target, name), [0]

    def wrapper(*a, **kw):
        seen[0] += 1
        if seen[0] == nth:
            raise Boom(f"{name} #{nth}")
        return real(*a, **kw)
    monkeypatch.setattr(target, name, wrapper)


@pytest.mark.parametrize("step", ["mkdir", "copy_header", "copy_rows", "meta", "files", "tombs", "fsync_dir",
                                  "manifest_tmp", "rename"])
def test_failure_before_the_commit_keeps_the_old_generation(tmp_path, monkeypatch, step):
    r, st, ids = build(tmp_path, CompactingIndex)
    CompactingIndex.calls.clear()
    man_before = open(os.path.join(st.path, "manifest.json")).read()
    data_before = st.index.data.copy()
    with monkeypatch.context() as m:
        if step == "mkdir":
            _fail_nth(m, os, "mkdir", 1)
        elif step == "copy_header":
            _fail_nth(m, rstore, "_copy_bytes", 1)
        elif step == "copy_rows":
            _fail_nth(m, rstore, "_copy_bytes", 3)
        elif step in ("meta", "files", "tombs"):
            _fail_nth(m, rstore, "_write_file", ("meta", "files", "tombs").index(step) + 1)
        elif step == "fsync_dir":
            _fail_nth(m, rstore, "_fsync_dir", 1)
        elif step == "manifest_tmp":
            _fail_nth(m, json, "dump", 1)
        else:
            _fail_nth(m, os, "replace", 1)
        with pytest.raises(Boom):
            st.compact()
    # nothing committed, nothing of this object touched, no device work
    assert open(os.path.join(st.path, "manifest.json")).read() == man_before
    assert CompactingIndex.calls == [] and np.array_equal(st.index.data, data_before, equal_nan=True)
    assert len(st.rows) == 12 and st.dead_rows() == 3
    assert not [n for n in os.listdir(st.path) if n.startswith("g-")], "the partial directory is removed"
    other = reg(tmp_path, CompactingIndex).get(st.name)
    assert other.index.rows == 12 and other.generation == st.generation  # opens as the old generation
    assert st.compact()["rows"] == 9  # and the next attempt goes through


def test_next_writer_removes_a_stray_generation_directory(tmp_path):
    r, st, ids = build(tmp_path, CompactingIndex)
    stray = os.path.join(st.path, "g-" + "0" * 32)  # a compaction that died before its manifest
    os.mkdir(stray)
    open(os.path.join(stray, "rows.rfx"), "wb").write(b"x" * 100)
    reg(tmp_path, CompactingIndex).get(st.name)  # readers leave it alone
    assert os.path.isdir(stray)
    st.add_document(["g0"], vecs(1, 8), "g.md")  # the next writer, under the lock
    assert not os.path.exists(stray)
    st.compact()
    os.mkdir(stray)
    st.delete_file(ids["A"])
    assert not os.path.exists(stray) and os.path.isdir(os.path.join(st.path, st.data_dir))


def test_reader_at_from_version_follows_on_its_index(tmp_path):
    a, st, ids = build(tmp_path, CompactingIndex)
    sb = reg(tmp_path, CompactingIndex).get(st.name)  # another process, caught up
    data = sb.index.data.copy()
    handle = sb.index
    evicted = []
    sb.on_compact.append(evicted.append)
    CompactingIndex.calls.clear()
    HostIndex.syncs.clear()
    st.compact()
    st.add_document(["F0", "F1"], vecs(2, 7), "F.md")  # and the generation moved on before the reader looked
    assert sb.stale() and sb.refresh()
    assert sb.index is handle, "the reader kept its index"
    assert CompactingIndex.calls == [[(0, 3), (5, 4), (10, 2)]] * 2  # the writer's and the reader's
    assert [s[1:] for s in HostIndex.syncs] == [(9, 11)], "only the rows appended afterwards were read"
    assert evicted == [st.name]
    assert sb.generation == st.generation and sb.version == st.version and sb.data_dir == st.data_dir
    assert [t for _, t in sb.rows] == KEPT_TEXT + ["F0", "F1"]
    assert np.array_equal(sb.index.data[:9], data[KEPT_ROWS]) and np.array_equal(sb.index.data, st.index.data)
    assert sb.files == st.files


def test_reader_a_version_behind_reloads(tmp_path):
    a, st, ids = build(tmp_path, CompactingIndex)
    sb = reg(tmp_path, CompactingIndex).get(st.name)
    st.delete_file(ids["E"])  # the reader does not see this one before the compaction
    CompactingIndex.calls.clear()
    HostIndex.syncs.clear()
    handle = sb.index
    st.compact()
    assert sb.refresh()
    assert sb.index is not handle and handle.closed
    assert CompactingIndex.calls == [[(0, 3), (5, 4)]]  # the writer's only
    assert [s[1:] for s in HostIndex.syncs] == [(0, 7)]
    assert [t for _, t in sb.rows] == KEPT_TEXT[:7] and np.array_equal(sb.index.data, st.index.data)


def test_reader_whose_generation_vanished_mid_catch_up_retries_once(tmp_path, monkeypatch):
    a, st, ids = build(tmp_path, PlainIndex)
    sb = reg(tmp_path, PlainIndex).get(st.name)
    st.add_document(["F0"], vecs(1, 7), "F.md")
    man, stat = sb._read_manifest()  # the reader has read this manifest ...
    st.delete_file(ids["E"])
    st.compact()                     # ... when a compaction removes the files it names
    with sb.lock:
        sb._sync(man, stat)
    assert sb.generation == st.generation and [t for _, t in sb.rows] == [t for _, t in st.rows]
    assert np.array_equal(sb.index.data, st.index.data)


# ---- hits in flight ---------------------------------------------------------------------------------------
def test_row_info_translates_the_previous_generation(tmp_path):
    r, st, ids = build(tmp_path, CompactingIndex)
    gen0 = st.generation
    before = {row: st.row_info(row) for row in range(12)}
    st.compact()
    gen1 = st.generation
    for row in range(12):
        got = st.row_info(row, generation=gen0)
        if row in KEPT_ROWS:
            assert got == before[row] and got == st.row_info(KEPT_ROWS.index(row))
        else:
            assert got is None, row  # a deleted row
    assert st.row_info(12, generation=gen0) is None and st.row_info(-1, generation=gen0) is None
    assert st.row_info(3, generation=gen1) == st.row_info(3) == before[5]
    assert st.numbering()[1] == gen1
    # one more compaction: gen0 is now older than the previous generation
    st.delete_file(ids["C"])
    st.compact()
    assert st.row_info(0, generation=gen0) is None
    assert st.row_info(7, generation=gen1)[1] == "E0" and st.row_info(3, generation=gen1) is None
    # a reader that reloaded has no map from the rows it dropped
    fresh = reg(tmp_path, CompactingIndex).get(st.name)
    assert fresh.row_info(0, generation=gen1) is None and fresh.row_info(0)[1] == "A0"


def test_numbering_token_changes_with_a_compaction(tmp_path):
    r, st, ids = build(tmp_path, CompactingIndex)
    token, gen = st.numbering()
    st.add_document(["x"], vecs(1, 3), "x.md")
    assert not st.numbering_changed(token)  # appends and deletes keep the numbering
    st.compact()
    assert st.numbering_changed(token) and st.numbering()[1] != gen


# ---- policy ---------------------------------------------------------------------------------------------------
def test_policy_off_by_default(tmp_path, monkeypatch):
    for v in ("RFX_COMPACT", "RFX_COMPACT_MIN_ROWS", "RFX_COMPACT_MIN_FRACTION"):
        monkeypatch.delenv(v, raising=False)
    assert rstore.compact_policy()[:2] == (False, 65536)
    monkeypatch.setenv("RFX_COMPACT_MIN_ROWS", "1")
    monkeypatch.setenv("RFX_COMPACT_MIN_FRACTION", "0.01")
    r, st, ids = build(tmp_path, CompactingIndex)
    gen = st.generation
    for k in "ACE":
        st.delete_file(ids[k])
    assert st.generation == gen and st.index.rows == 12 and st.data_dir is None


def test_policy_auto_triggers_exactly_at_both_thresholds(tmp_path, monkeypatch):
    monkeypatch.setenv("RFX_COMPACT", "auto")
    monkeypatch.setenv("RFX_COMPACT_MIN_ROWS", "4")
    monkeypatch.setenv("RFX_COMPACT_MIN_FRACTION", "0.5")
    r = reg(tmp_path, CompactingIndex)
    st = r.create("demo", 64, "f32")
    ids = [st.add_document([f"{i}{j}" for j in range(2)], vecs(2, i), f"{i}.md")[0] for i in range(6)]  # 12 rows
    gen = st.generation
    st.delete_file(ids[0])  # 2 dead: below both
    st.delete_file(ids[1])  # 4 dead of 12: the row threshold holds, the fraction (6) does not
    assert st.generation == gen and st.dead_rows() == 4
    monkeypatch.setenv("RFX_COMPACT_MIN_ROWS", "7")
    st.delete_file(ids[2])  # 6 dead of 12: the fraction holds, the row threshold (7) does not
    assert st.generation == gen and st.dead_rows() == 6
    monkeypatch.setenv("RFX_COMPACT_MIN_ROWS", "8")
    monkeypatch.setenv("RFX_COMPACT_MIN_FRACTION", "0.6666")
    st.delete_file(ids[3])  # 8 dead of 12: exactly at both
    assert st.generation != gen and st.index.rows == 4 and st.dead_rows() == 0
    assert [t for _, t in st.rows] == ["40", "41", "50", "51"]
    assert reg(tmp_path, CompactingIndex).get(st.name).index.rows == 4


def test_policy_auto_failure_never_fails_the_delete(tmp_path, monkeypatch, caplog):
    monkeypatch.setenv("RFX_COMPACT", "auto")
    monkeypatch.setenv("RFX_COMPACT_MIN_ROWS", "1")
    monkeypatch.setenv("RFX_COMPACT_MIN_FRACTION", "0.01")
    r = reg(tmp_path, CompactingIndex)
    st = r.create("demo", 64, "f32")
    ids = [st.add_document(["a", "b"], vecs(2, i), f"{i}.md")[0] for i in range(3)]
    gen = st.generation
    _fail_nth(monkeypatch, rstore, "_write_file", 1)
    with caplog.at_level("WARNING", logger="rfx.store"):
        assert st.delete_file(ids[0]) is True
    assert st.generation == gen and st.files[ids[0]]["deleted"] and st.index.rows == 6
    assert any("compaction" in rec.getMessage() for rec in caplog.records)
    assert reg(tmp_path, CompactingIndex).get(st.name).files[ids[0]]["deleted"]


# ---- the registry's hook: views and batchers built over the old numbering go ---------------------------------
def test_registry_runs_its_eviction_callbacks_on_compaction(tmp_path):
    r, st, ids = build(tmp_path, CompactingIndex)
    seen = []
    r.on_evict.append(seen.append)
    st.compact()
    assert seen == [st.name]
    assert r.get(st.name) is st  # the store itself stays in the registry
