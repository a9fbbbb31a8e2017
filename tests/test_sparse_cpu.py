"""CPU checks of the sparse-result entry points (fora_hip_query_sparse_batch / fora_hip_sparse_fetch /
fora_hip_sparse_clear): declared, exported, bound; a NULL context is refused without a GPU; the compaction kernels are
in the shipped code object without scratch or spills.  (The C layout of fora_sparse_stats, as of every struct:
tests/test_capi_cpu.py.)"""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
NAMES = ("fora_hip_query_sparse_batch", "fora_hip_sparse_fetch", "fora_hip_sparse_clear")
FORA_E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    return capi.load()


def test_declared_exported_and_bound(lib):
    from fora_amd import capi
    text = open(os.path.join(ROOT, "include", "fora_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS, name
    assert "fora_sparse_stats" in text
    assert callable(getattr(capi.Engine, "query_sparse", None)) and callable(getattr(capi.Engine, "sparse_clear", None))
    assert callable(getattr(capi, "to_torch_csr", None))


def test_null_context_is_refused_without_a_gpu(lib):
    src = (ctypes.c_int32 * 2)(0, 1)
    row_ptr = (ctypes.c_int64 * 3)(7, 7, 7)
    assert lib.fora_hip_query_sparse_batch(None, src, 2, 0, 0.0, row_ptr, None, None) == FORA_E_ARG
    assert list(row_ptr) == [7, 7, 7]
    ids = (ctypes.c_int32 * 4)(9, 9, 9, 9)
    assert lib.fora_hip_sparse_fetch(None, ids, None, None, 4) == FORA_E_ARG
    assert list(ids) == [9, 9, 9, 9]
    assert lib.fora_hip_sparse_clear(None) == FORA_E_ARG


def test_compaction_kernels_are_shipped_without_scratch():
    import isa_audit
    from fora_amd import build
    rows = {r["kernel"]: r for r in isa_audit.audit(build.build_hip())}
    for k in ("k_sparse_count", "k_sparse_write", "k_sparse_single", "k_sparse_vals"):
        assert k in rows, (k, sorted(rows))
        assert rows[k]["scratch_bytes"] == 0 and rows[k]["vgpr_spill"] == 0 and rows[k]["sgpr_spill"] == 0, rows[k]
