"""Sparse rows and sweep cuts for seed sets, on CPU: the header names the two contracts and declares the entry points, both
libraries export them and answer a NULL ctx without a GPU, fora_amd.capi binds them; and, on rows of the CPU twin, the
property the feature exists for -- a threshold applied after the sum keeps a node that every per-seed thresholded row has
lost.  The GPU runs are in test_seeds_sparse_gpu.py and test_seeds_sweep_gpu.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import seeds_outputs_ref as so
import seeds_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPARSE = "fora_hip_seeds_sparse_batch"
SWEEP = "fora_hip_seeds_sweep_batch"
SETS = ["fora_ctx *ctx", "const int64_t *set_ptr", "const int32_t *seeds", "const double *weights", "int ns", "int with_idx"]


def _declared(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, f"{name}: no declaration"
    return [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]  # (comments hold commas)


def test_header_names_the_two_blocks_and_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "fora_hip.h")).read()
    assert " * SEED SETS, SPARSE (" + SPARSE + ")" in hdr and " * SEED SETS, SWEPT (" + SWEEP + ")" in hdr
    assert _declared(hdr, SPARSE) == SETS + ["double threshold", "int64_t *row_ptr", "uint64_t *row_sum_fix_out",
                                            "fora_seeds_stats *st", "fora_sparse_stats *sp"]
    assert _declared(hdr, SWEEP) == SETS + ["double threshold", "int64_t max_size", "int64_t *row_ptr", "fora_sweep_row *rows",
                                           "fora_seeds_stats *st", "fora_sweep_stats *sw"]
    # the lifetime sentences of the two result blocks list the new calls
    assert re.search(r"until the next\s+\*?\s*fora_hip_query_sparse_batch or " + SPARSE, hdr)
    assert re.search(r"until the next fora_hip_sweep_batch or " + SWEEP, hdr)


def test_capi_binds_them_and_the_engine_has_the_methods():
    from fora_amd import capi
    assert SPARSE in capi.SYMBOLS and SWEEP in capi.SYMBOLS
    assert SPARSE not in capi.TEST_SYMBOLS and SWEEP not in capi.TEST_SYMBOLS and len(capi.TEST_SYMBOLS) == 5
    want = {
        "query_seeds_sparse": (["self", "sets", "weights", "with_idx", "threshold", "want_fix", "device"],
                               (None, False, None, False, False)),
        "sweep_seeds": (["self", "sets", "weights", "with_idx", "threshold", "max_size", "want_profile", "device"],
                        (None, False, None, 0, False, False)),
    }
    for name, (params, defaults) in want.items():
        sig = inspect.signature(getattr(capi.Engine, name))
        assert list(sig.parameters) == params, name
        assert tuple(p.default for p in list(sig.parameters.values())[2:]) == defaults, name
    sig = inspect.signature(capi.Engine.local_cluster_seeds)
    assert list(sig.parameters)[:3] == ["self", "sets", "weights"] and sig.parameters["weights"].default is None


def test_the_option_is_in_the_table_and_in_the_integration_guide():
    src = open(os.path.join(ROOT, "fora_amd", "csrc", "fora_hip.hip")).read()
    assert re.search(r"int64_t seeds_rows = 256;", src) and '{"seeds_rows", &Tunables::seeds_rows, false}' in src
    assert "`seeds_rows=" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


@pytest.mark.parametrize("which", ["lib", "test_lib"])
def test_libraries_export_them_and_a_null_ctx_is_an_argument_error(which):
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    lib = capi.load(None if which == "lib" else capi.TEST_LIB)
    sp, sw = getattr(lib, SPARSE), getattr(lib, SWEEP)
    row_ptr = np.full(2, -5, dtype=np.int64)
    rp = row_ptr.ctypes.data_as(ctypes.c_void_p)
    # FORA_E_ARG, answered without a GPU, nothing written
    assert sp(None, None, None, None, 0, 0, 0.0, rp, None, None, None) == -1
    assert sw(None, None, None, None, 0, 0, 0.0, 0, rp, None, None, None) == -1
    assert (row_ptr == -5).all()


def test_the_sum_keeps_a_node_that_every_thresholded_seed_row_has_lost(oracle, tiny):
    """A uniform 3-seed set on rows of the CPU twin.  There is a node v and a threshold thr with every term
    floor(wfix_j * x_j[v] / 2^62) < thr <= row[v]: thresholding after the sum keeps v, and the merge of the per-seed
    thresholded rows -- the only route to a sparse set row before these entry points -- does not hold v at all."""
    g = tiny
    rmax, omega = oracle.fora_setting(g.n, g.m, so.EPS, alpha=so.ALPHA)
    seeds = so.pick(g, 3, 611)
    assert len(set(seeds)) == 3
    rows = [oracle.twin_query(g, s, rmax, omega, alpha=so.ALPHA, seed=so.SEED)[0].tolist() for s in seeds]
    wfix = sr.uniform_wfix(3)
    row = sr.combine(rows, wfix)
    found = so.lifted_node(rows, wfix)
    assert found is not None, "no node with two or more non-zero terms"
    v, thr, terms = found
    assert thr == row[v] == sum(terms) and sum(1 for t in terms if t) >= 2
    assert all(t < thr for t in terms) and thr <= row[v]
    kept = so.csr_of([row], thr)
    assert v in kept[1] and kept[2][kept[1].index(v)] == row[v]
    merged = so.merge_thresholded(rows, wfix, thr)
    assert v not in merged
    # ... and what the merge does hold is never more than the row: mass under the threshold in a seed's row is simply gone
    assert all(x <= row[u] for u, x in merged.items())
    assert float(thr) == thr and so.thr_fix_of(float(thr) * 2.0 ** -62) == thr  # a call can ask for exactly this threshold
