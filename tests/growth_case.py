"""The input of the two test_growth_with_entries_to_keep (tests/test_sparse_gpu.py, tests/test_sweep_gpu.py): a call whose held
arrays must grow in the middle, with entries already written to carry over.  Chosen once, from the dense rows."""
import numpy as np

from conftest import pick_sources

SEED = 0x464F5241


def _load(engine, g):
    engine.clear_index()
    engine.set_graph(g.n, g.m, g.row_ptr, g.col)
    engine.set_params(seed=SEED, epsilon=0.5)


def growths_with_entries_to_keep(lens):
    """How often a call over rows of these lengths, one row per batch, starting from empty held arrays, has to grow them
    while entries already written must be carried over.  The growth rule restated: the first capacity comes from row 1;
    after rows_done of rows_all rows, need entries that do not fit ask for max(need, need / rows_done * rows_all * 1.125 + 1024)."""
    cap = need = kept = 0
    for done, length in enumerate(lens, 1):
        written = need
        need += int(length)
        if need > cap:
            kept += written > 0
            cap = max(need, int(need / done * len(lens) * 1.125) + 1024, 1)
    return kept


class _Csr:
    def __init__(self, n, m, row_ptr, col):
        self.n, self.m = int(n), int(m)
        self.row_ptr, self.col = np.ascontiguousarray(row_ptr, dtype=np.int64), np.ascontiguousarray(col, dtype=np.int32)
        self.deg = np.diff(self.row_ptr)


_GROWTH = {}


def growth_case(engine, small):
    """(g, srcs): the `small` preset with a two-node cycle appended as a component of its own -- a source there has a row of
    exactly 2 entries at threshold 0 -- and six sources: a node of the cycle, then five of the preset whose dense rows have
    the most non-zeros among 32 candidates, the shortest first.  With one row per batch such a call grows its held arrays
    at least twice with written entries to carry over (asserted, from the dense rows' lengths).  Leaves g loaded."""
    if not _GROWTH:
        n, nnz = small.n, int(small.row_ptr[-1])
        g = _Csr(n + 2, small.m + 2, np.concatenate([small.row_ptr, [nnz + 1, nnz + 2]]), np.concatenate([small.col, [n + 1, n]]))
        _load(engine, g)
        cand = pick_sources(small, 32, 4250)
        rows, _, _ = engine.query_fix(cand)
        nz = (rows != 0).sum(axis=1)
        top = np.argsort(nz, kind="stable")[-5:]
        _GROWTH["case"] = (g, np.concatenate([[n], cand[top]]).astype(np.int32))
        print("growth case: candidates' non-zeros min %d median %d max %d; chosen %s" % (nz.min(), np.median(nz), nz.max(), nz[top].tolist()))
    g, srcs = _GROWTH["case"]
    _load(engine, g)
    return g, srcs
