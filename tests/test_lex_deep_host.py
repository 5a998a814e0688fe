"""CPU: the deep lexical entry points are declared, exported and bound; parse_hybrid_deep's range."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rfx_lex_search_deep_workspace_bytes", "rfx_lex_search_deep", "rfx_lex_fuse_deep")


def test_symbols_are_declared_exported_and_bound():
    from rfx import _lib, lexical
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "rfx.h")).read()
    for s in SYMBOLS:
        assert s in exported and s in _lib.SIGNATURES and re.search(r"^int %s\(" % s, header, re.M), s
    for name in ("search_deep", "deep_workspace_bytes", "fuse_deep"):
        assert callable(getattr(lexical.LexIndex, name))


def test_parse_hybrid_deep_argument():
    from rfx.retriever import parse_hybrid, parse_hybrid_deep
    assert parse_hybrid_deep(None, 100) is None
    assert parse_hybrid_deep(0.25, 100) == (0.25, 100, 60, 1.2, 0.75)  # fetch_k defaults to k
    for fetch_k in (65, 100, 1024):
        got = parse_hybrid_deep({"alpha": 1, "fetch_k": fetch_k, "rrf_c": 10, "k1": 0.9, "b": 0.5}, 65)
        assert got == (1.0, fetch_k, 10, 0.9, 0.5)
    for bad in ({"alpha": 0.5, "fetch_k": 99}, {"alpha": 0.5, "fetch_k": 1025}, {"alpha": 0.5, "fetch_k": 200.0},
                {"fetch_k": 200}, 1.5, float("nan"), {"alpha": 0.5, "rrf_c": 0}, {"alpha": 0.5, "b": 2.0},
                {"alpha": 0.5, "k1": -1.0}, {"alpha": 0.5, "beta": 1}):
        with pytest.raises(ValueError):
            parse_hybrid_deep(bad, 100)
    with pytest.raises(ValueError):  # the shallow parser keeps its limit
        parse_hybrid({"alpha": 0.5, "fetch_k": 65}, 10)
