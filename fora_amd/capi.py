"""ctypes binding of libfora_hip.so (include/fora_hip.h).  Thin: every method is
one C-ABI call; errors raise ForaError with fora_hip_last_error().

The C ABI is stated once here: the struct mirrors, and _ABI, one row per function, which load() binds (restype and
argtypes) on whatever the library exports -- so a call passes plain Python values and ctypes converts, or refuses,
each of them.  A new entry point takes three steps: its prototype in include/fora_hip.h, its row in _ABI (a struct of
its own: a mirror in STRUCTS), one Engine method.  tests/test_capi_cpu.py derives every row and every mirror from the
header again and fails until they match.  Entry points declared in the extension header include/fora_hip_ext.h have
their rows in a second table, _ABI_EXT, of the same syntax, bound by the same load() (tests/test_subgraph_cpu.py holds
it to that header); they report statistics through out-pointers and add no struct.  The entry points of
include/fora_hip_gnn.h (message passing on the held subgraph) have a third table of the same kind, _ABI_GNN
(tests/test_subgraph_prop_cpu.py)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
FIX_ONE = 1 << 62
STREAM_INDEX = 0xFFFFFFFF
BWD_FIX_ONE = 1 << 60


class ForaError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"fora_hip error {code}: {msg}")
        self.code = code


# ---- the C ABI: the types of include/fora_hip.h by the names the rows below use.  Every data pointer is "ptr" (c_void_p:
# host or device memory, or a scalar out-parameter; it takes _p(array), byref(x), a data_ptr() integer and None), a
# pointer to a fora_* struct is POINTER(its mirror) ("sparse_stats*": an array of the mirror, a byref or None)
_TYPES = {"void": None, "int": C.c_int, "int32": C.c_int32, "uint32": C.c_uint32, "int64": C.c_int64, "uint64": C.c_uint64,
          "double": C.c_double, "str": C.c_char_p, "ptr": C.c_void_p, "ctx*": C.c_void_p, "ctx**": C.POINTER(C.c_void_p)}


def _fields(spec):
    """the _fields_ of a mirror from its declaration, "uint64 entries max_row; int32 batches" """
    return [(name, _TYPES[t]) for t, *names in (part.split() for part in spec.split(";")) for name in names]


class _Stats(C.Structure):
    """a mirror that reads out as a dict; padding (a name that ends in "_": reserved_, pad_) is left out"""

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.endswith("_")}


def _np_dtype(mirror):
    """the structured numpy dtype of an array of a mirror (st[i]["pops"] as on a list of dicts)"""
    dt = np.dtype([(name, np.dtype(ct)) for name, ct in mirror._fields_], align=True)
    assert dt.itemsize == C.sizeof(mirror)
    return dt


class QueryStats(C.Structure):
    _fields_ = _fields("double rsum; uint64 rsum_fix n_rw n_walks n_idx_hit pops relax ppr_sum_fix; int32 levels dangling_source;"
                       "double rmax_used; int32 push_rounds reserved_")


class Timing(_Stats):
    _fields_ = _fields("double push_pop_ms push_expand_ms push_accum_ms walk_alloc_ms walk_ms walk_accum_ms other_ms batch_ms;"
                       "uint64 push_pop_launches push_expand_launches push_accum_launches walk_launches batches pops relax walks"
                       " walk_steps levels idx_hits; double push_tail_ms; uint64 push_tail_launches; double push_team_ms;"
                       "uint64 push_team_launches")


class BwdStats(_Stats):
    _fields_ = _fields("uint64 targets pops relax entries global_targets; int32 levels chunks; double bwd_ms walk_ms combine_ms")


class SparseStats(_Stats):
    _fields_ = _fields("uint64 entries max_row thr_fix; int32 batches reserved_; double compact_ms")


class TopkStats(_Stats):
    _fields_ = _fields("uint64 support max_support k; int32 cut_rows lds_rows global_rows chunks; double select_ms")


class SeedsStats(_Stats):
    _fields_ = _fields("uint64 seeds distinct queries dangling; int32 batches reserved_; double combine_ms")


class SweepRow(C.Structure):
    _fields_ = _fields("int64 len best; uint64 cut vol den; double conductance")


class SweepStats(_Stats):
    _fields_ = _fields("uint64 entries max_row thr_fix edges; int32 batches global_rows; double compact_ms sort_ms cut_ms")


class PropStats(_Stats):
    _fields_ = _fields("uint64 entries segments max_row feat_bytes; int32 chunks feat_on_device; double gather_ms combine_ms")


class PropTStats(_Stats):
    _fields_ = _fields("uint64 entries columns segments max_col feat_bytes;"
                       "int32 chunks feat_on_device built short_cols lds_cols global_cols; double transpose_ms gather_ms combine_ms")


class SddmmStats(_Stats):
    _fields_ = _fields("uint64 entries segments max_row bytes; int32 a_on_device b_on_device; double sddmm_ms")


class SoftmaxStats(_Stats):
    _fields_ = _fields("uint64 entries segments max_row nan_rows short_rows long_rows; int32 in_on_device grad_on_device;"
                       "double softmax_ms")


class AttnStats(_Stats):
    _fields_ = _fields("uint64 entries segments max_row nan_rows short_rows long_rows;"
                       "int32 q_on_device k_on_device v_on_device pad_; double attn_ms")


class AttnGrads(C.Structure):
    """fora_attn_grads: the outputs of fora_hip_sparse_attention_bwd, each gradient as f32 and / or f64 with one pitch"""
    _fields_ = _fields("ptr dq32 dq64; int64 lddq; ptr dk32 dk64; int64 lddk; ptr dv32 dv64; int64 lddv")


class AttnBwdStats(_Stats):
    _fields_ = _fields("uint64 entries segments max_row short_rows long_rows columns max_col short_cols long_cols;"
                       "int32 built plan_cached q_on_device k_on_device v_on_device g_on_device y_on_device pad_;"
                       "double transpose_ms attn_ms")


class StoreStats(_Stats):
    _fields_ = _fields("uint64 rows entries max_row store_rows store_entries; int32 ids_on_device fix_on_device; double store_ms")


class ColsStats(_Stats):
    _fields_ = _fields("uint64 entries cols words; double cols_ms")


_STATS_DTYPE, _SWEEP_ROW_DTYPE = _np_dtype(QueryStats), _np_dtype(SweepRow)
STRUCTS = {"fora_query_stats": QueryStats, "fora_timing": Timing, "fora_bwd_stats": BwdStats, "fora_sparse_stats": SparseStats,
           "fora_seeds_stats": SeedsStats, "fora_sweep_row": SweepRow, "fora_sweep_stats": SweepStats, "fora_prop_stats": PropStats,
           "fora_propt_stats": PropTStats, "fora_sddmm_stats": SddmmStats, "fora_softmax_stats": SoftmaxStats,
           "fora_attn_stats": AttnStats, "fora_attn_grads": AttnGrads, "fora_attn_bwd_stats": AttnBwdStats,
           "fora_store_stats": StoreStats, "fora_cols_stats": ColsStats, "fora_topk_stats": TopkStats}
_TYPES.update({name[len("fora_"):] + "*": C.POINTER(mirror) for name, mirror in STRUCTS.items()})

# one row per function, as the header declares it without the parameter names; "test": one of the TEST ENTRY POINTS of
# include/fora_hip.h, in libfora_hip_test.so (TEST_LIB) only
_ABI = """
int  fora_hip_device_count()
int  fora_hip_create(int, ctx**)
void fora_hip_destroy(ctx*)
str  fora_hip_last_error(ctx*)
int  fora_hip_device_info(ctx*, str, int, ptr, ptr)
int  fora_hip_set_graph(ctx*, int32, int64, ptr, ptr)
int  fora_hip_set_params(ctx*, double, double, double, int, uint64)
int  fora_hip_set_params_raw(ctx*, double, double, double, int, uint64)
int  fora_hip_get_params(ctx*, ptr, ptr)
int  fora_hip_set_balanced(ctx*, int, double, double, double, double, double)
int  fora_hip_set_batch(ctx*, int)
int  fora_hip_get_batch(ctx*)
int  fora_hip_set_option(ctx*, str, int64)
int  fora_hip_get_option(ctx*, str, ptr)
int  fora_hip_index_sizes(ctx*, ptr, ptr, ptr)
int  fora_hip_build_index(ctx*)
int  fora_hip_get_index(ctx*, ptr, uint64, ptr, ptr)
int  fora_hip_set_index(ctx*, ptr, uint64, ptr, ptr)
int  fora_hip_clear_index(ctx*)
int  fora_hip_query_batch(ctx*, ptr, int, int, ptr, query_stats*)
int  fora_hip_query_batch_fix(ctx*, ptr, int, int, ptr, ptr, query_stats*)
int  fora_hip_query_sparse_batch(ctx*, ptr, int, int, double, ptr, query_stats*, sparse_stats*)
int  fora_hip_sparse_fetch(ctx*, ptr, ptr, ptr, uint64)
int  fora_hip_sparse_clear(ctx*)
int  fora_hip_sparse_propagate(ctx*, ptr, int, ptr, int, int, int64, int, ptr, ptr, int64, prop_stats*)
int  fora_hip_sparse_propagate_t(ctx*, ptr, int, ptr, int, int, int64, int, ptr, ptr, int64, propt_stats*)
int  fora_hip_sparse_propagate_vals(ctx*, ptr, int, ptr, int, int, int64, int, ptr, int, ptr, ptr, int64, prop_stats*)
int  fora_hip_sparse_propagate_t_vals(ctx*, ptr, int, ptr, int, int, int64, int, ptr, int, ptr, ptr, int64, propt_stats*)
int  fora_hip_sparse_sddmm(ctx*, ptr, int, ptr, int, int64, ptr, int, int64, int, ptr, ptr, uint64, sddmm_stats*)
int  fora_hip_sparse_softmax(ctx*, ptr, int, ptr, int, double, ptr, ptr, uint64, softmax_stats*)
int  fora_hip_sparse_softmax_bwd(ctx*, ptr, int, ptr, int, ptr, int, double, ptr, ptr, uint64, softmax_stats*)
int  fora_hip_sparse_attention(ctx*, ptr, int, ptr, int, int64, ptr, int, int64, ptr, int, int64, int, int, int, double, ptr, ptr, int64, ptr, ptr, uint64, attn_stats*)
int  fora_hip_sparse_attention_bwd(ctx*, ptr, int, ptr, int, int64, ptr, int, int64, ptr, int, int64, ptr, int, int64, ptr, int, uint64, int, int, int, double, attn_grads*, attn_bwd_stats*)
int  fora_hip_sparse_transpose_fetch(ctx*, ptr, int, ptr, ptr, ptr, ptr, uint64)
int  fora_hip_store_put(ctx*, ptr, int, int, store_stats*)
int  fora_hip_store_load(ctx*, ptr, int64, ptr, ptr, int, store_stats*)
int  fora_hip_store_take(ctx*, ptr, int, ptr, store_stats*)
int  fora_hip_store_info(ctx*, ptr, ptr, ptr)
int  fora_hip_store_clear(ctx*)
int  fora_hip_sparse_compact(ctx*, ptr, int, ptr, cols_stats*)
int  fora_hip_sparse_cols_fetch(ctx*, ptr, uint64)
int  fora_hip_sweep_batch(ctx*, ptr, int, int, double, int64, ptr, sweep_row*, query_stats*, sweep_stats*)
int  fora_hip_sweep_fetch(ctx*, ptr, ptr, ptr, uint64)
int  fora_hip_sweep_clear(ctx*)
int  fora_hip_query_seeds_batch(ctx*, ptr, ptr, ptr, int, int, ptr, ptr, int, ptr, ptr, ptr, seeds_stats*)
int  fora_hip_seeds_sparse_batch(ctx*, ptr, ptr, ptr, int, int, double, ptr, ptr, seeds_stats*, sparse_stats*)
int  fora_hip_query_sparse_topk_batch(ctx*, ptr, int, int, double, int64, ptr, query_stats*, sparse_stats*, topk_stats*)
int  fora_hip_seeds_sparse_topk_batch(ctx*, ptr, ptr, ptr, int, int, double, int64, ptr, ptr, seeds_stats*, sparse_stats*, topk_stats*)
int  fora_hip_seeds_sweep_batch(ctx*, ptr, ptr, ptr, int, int, double, int64, ptr, sweep_row*, seeds_stats*, sweep_stats*)
int  fora_hip_topk_batch(ctx*, ptr, int, int, double, double, int, ptr, ptr, ptr)
int  fora_hip_topk_bound_batch(ctx*, ptr, int, int, double, double, double, int, ptr, ptr, ptr)
int  fora_hip_power_iteration_batch(ctx*, ptr, int, int, ptr, ptr, int, ptr, ptr)
int  fora_hip_montecarlo_batch(ctx*, ptr, int, double, ptr, ptr, int, ptr, ptr, query_stats*)
int  fora_hip_fwdpush_batch(ctx*, ptr, int, double, double, ptr, ptr, ptr, int, ptr, ptr, query_stats*)
int  fora_hip_bippr_batch(ctx*, ptr, int, double, double, ptr, ptr, int, ptr, ptr, query_stats*, bwd_stats*)
int  fora_hip_bippr_targets_batch(ctx*, ptr, int, ptr, int, double, double, ptr, ptr, query_stats*, bwd_stats*)
int  fora_hip_push_batch(ctx*, ptr, int, ptr, ptr, query_stats*)
int  fora_hip_bwdpush_batch(ctx*, ptr, int, double, ptr, ptr, bwd_stats*)
int  fora_hip_walk_counts(ctx*, ptr, double, ptr, ptr)
int  fora_hip_walks(ctx*, uint32, uint32, int, ptr, ptr, int64, ptr)
int  fora_hip_reset_timing(ctx*)
int  fora_hip_get_timing(ctx*, timing*)
int  fora_hip_get_stamps(ctx*, ptr)
test int fora_hip_test_sweep_rows(ctx*, ptr, int, double, int64, ptr, sweep_row*, sweep_stats*)
test int fora_hip_test_sparse_rows(ctx*, ptr, int, double, ptr, sparse_stats*)
test int fora_hip_test_sparse_topk_rows(ctx*, ptr, int, double, int64, ptr, sparse_stats*, topk_stats*)
test int fora_hip_test_sweep_scan(ctx*, ptr, ptr, int64, uint64, ptr)
test int fora_hip_test_exp(ctx*, ptr, int64, ptr)
"""


def _rows(text):
    """{name: (test_only, restype, argtypes)} of the rows of _ABI"""
    out = {}
    for row in text.strip().splitlines():
        *mark, ret, sig = row.split(None, 2) if row.startswith("test ") else row.split(None, 1)
        name, args = sig.rstrip(")").split("(")
        out[name] = (bool(mark), _TYPES[ret], [_TYPES[a] for a in args.split(", ") if a])
    return out


ABI = _rows(_ABI)
SYMBOLS = [name for name, row in ABI.items() if not row[0]]
TEST_SYMBOLS = [name for name, row in ABI.items() if row[0]]  # TEST_LIB only

# the entry points of include/fora_hip_ext.h, the extension header: the same rows, a table of their own (the census of
# include/fora_hip.h is pinned); tests/test_subgraph_cpu.py derives them from that header again
_ABI_EXT = """
int  fora_hip_sparse_subgraph(ctx*, ptr, int, ptr, ptr, ptr)
int  fora_hip_sparse_subgraph_fetch(ctx*, ptr, ptr, ptr, uint64)
"""
ABI_EXT = _rows(_ABI_EXT)
EXT_SYMBOLS = list(ABI_EXT)

# the entry points of include/fora_hip_gnn.h, message passing on the held subgraph: a third table of the same syntax (the
# censuses of the two headers above are pinned); tests/test_subgraph_prop_cpu.py derives them from that header again
_ABI_GNN = """
int  fora_hip_subgraph_propagate(ctx*, ptr, int, int, int64, int, ptr, int, ptr, ptr, int64, ptr, ptr)
int  fora_hip_subgraph_propagate_t(ctx*, ptr, int, int, int64, int, ptr, int, ptr, ptr, int64, ptr, ptr)
int  fora_hip_subgraph_transpose_fetch(ctx*, ptr, ptr, ptr, uint64)
"""
ABI_GNN = _rows(_ABI_GNN)
GNN_SYMBOLS = list(ABI_GNN)
SUB_MEAN = 1  # FORA_SUB_MEAN


PROP_SEG = 256  # FORA_PROP_SEG
PROP_F32, PROP_BF16, PROP_F64 = 0, 1, 2  # (PROP_F64: the values of the *_vals calls only)
PROP_F16, PROP_E4M3, PROP_E5M2 = 4, 5, 6  # (NARROW OPERANDS of include/fora_hip.h: legal where PROP_BF16 is; 3 is no type)
PROP_NORMALIZE = 1


def to_torch_csr(row_ptr, ids, vals, n):
    """The [nq, n] torch.sparse_csr_tensor of a device result of Engine.query_sparse (column ids widened to int64 to
    match row_ptr)."""
    import torch
    return torch.sparse_csr_tensor(row_ptr, ids.to(torch.int64), vals, size=(row_ptr.numel() - 1, int(n)))


def subgraph_edge_index(sub_ptr, sub_col):
    """The [2, edges] COO pair (source, target; int64, local ids) of a CSR of Engine.sparse_subgraph: numpy arrays give a
    numpy array, torch tensors a tensor on their device."""
    if type(sub_ptr).__module__.split(".")[0] == "torch":
        import torch
        rows = torch.arange(sub_ptr.numel() - 1, dtype=torch.int64, device=sub_ptr.device)
        return torch.stack([torch.repeat_interleave(rows, sub_ptr[1:] - sub_ptr[:-1]), sub_col.to(torch.int64)])
    sub_ptr = np.asarray(sub_ptr, dtype=np.int64)
    return np.stack([np.repeat(np.arange(sub_ptr.size - 1, dtype=np.int64), np.diff(sub_ptr)), np.asarray(sub_col, dtype=np.int64)])


def lib_path():
    # FORA_HIP_LIB: experiment tooling only (tools/pushbench.py times several builds of the library)
    return os.environ.get("FORA_HIP_LIB") or os.path.join(_HERE, "libfora_hip.so")


TEST_LIB = os.path.join(_HERE, "libfora_hip_test.so")  # -DFORA_TEST_PATHS=1: threshold rounds / bounded deferral compiled in
_LIBS = {}


def _bind(lib):
    """restype and argtypes of every row of the ABI the library exports; a symbol it lacks (a test entry point in the
    product library, a newer call in an older build under FORA_HIP_LIB) stays unbound and raises AttributeError on use"""
    for name, (_, restype, argtypes) in list(ABI.items()) + list(ABI_EXT.items()) + list(ABI_GNN.items()):
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return lib


def load(path=None):
    """Loads the in-tree HIP library (path: another build of it -- libfora_hip_test.so, the build with the schedule
    experiments compiled in, for their twin-equivalence tests).  Fails loudly when it has not been built."""
    path = path or lib_path()
    if path not in _LIBS:
        if not os.path.exists(path):
            raise ImportError(f"{path} missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _LIBS[path] = _bind(C.CDLL(path))
    return _LIBS[path]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Engine:
    """One GPU context (fora_ctx)."""

    def __init__(self, device=0, lib=None):
        self._lib = load(lib)
        self._ctx = C.c_void_p()
        rc = self._lib.fora_hip_create(device, C.byref(self._ctx))
        if rc:
            raise ForaError(rc, "fora_hip_create failed (no gfx950 GPU visible?)")
        self.n = 0
        self.device = int(device)

    def close(self):
        if self._ctx:
            self._lib.fora_hip_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise ForaError(rc, (self._lib.fora_hip_last_error(self._ctx) or b"").decode())

    def device_info(self):
        arch = C.create_string_buffer(64)
        cus, hbm = C.c_int(0), C.c_uint64(0)
        self._chk(self._lib.fora_hip_device_info(self._ctx, arch, 64, C.byref(cus), C.byref(hbm)))
        return arch.value.decode(), cus.value, hbm.value

    def set_graph(self, n, m_attr, row_ptr, col):
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64)
        col = np.ascontiguousarray(col, dtype=np.int32)
        self._chk(self._lib.fora_hip_set_graph(self._ctx, n, m_attr, _p(row_ptr), _p(col)))
        self.n = int(n)

    def set_params(self, alpha=0.2, epsilon=0.5, rmax_scale=1.0, opt=False, seed=0):
        self._chk(self._lib.fora_hip_set_params(self._ctx, alpha, epsilon, rmax_scale, int(opt), seed))

    def set_params_raw(self, alpha, rmax, omega, opt=False, seed=0):
        self._chk(self._lib.fora_hip_set_params_raw(self._ctx, alpha, rmax, omega, int(opt), seed))

    def get_params(self):
        rmax, omega = C.c_double(0), C.c_double(0)
        self._chk(self._lib.fora_hip_get_params(self._ctx, C.byref(rmax), C.byref(omega)))
        return rmax.value, omega.value

    def set_batch(self, batch):
        self._chk(self._lib.fora_hip_set_batch(self._ctx, batch))

    def get_batch(self):
        return self._lib.fora_hip_get_batch(self._ctx)

    # ---- index
    def index_sizes(self):
        total = C.c_uint64(0)
        off = np.zeros(self.n, dtype=np.uint64)
        cnt = np.zeros(self.n, dtype=np.uint64)
        self._chk(self._lib.fora_hip_index_sizes(self._ctx, C.byref(total), _p(off), _p(cnt)))
        return total.value, off, cnt

    def build_index(self):
        self._chk(self._lib.fora_hip_build_index(self._ctx))

    def get_index(self):
        total, _, _ = self.index_sizes()
        rw = np.zeros(max(1, total), dtype=np.int32)
        off = np.zeros(self.n, dtype=np.uint64)
        cnt = np.zeros(self.n, dtype=np.uint64)
        self._chk(self._lib.fora_hip_get_index(self._ctx, _p(rw), total, _p(off), _p(cnt)))
        return rw[:total], off, cnt

    def set_index(self, rw_idx, off, cnt):
        rw_idx = np.ascontiguousarray(rw_idx, dtype=np.int32)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        cnt = np.ascontiguousarray(cnt, dtype=np.uint64)
        self._chk(self._lib.fora_hip_set_index(self._ctx, _p(rw_idx), rw_idx.size, _p(off), _p(cnt)))

    def clear_index(self):
        self._chk(self._lib.fora_hip_clear_index(self._ctx))

    # ---- queries
    @staticmethod
    def _stats(arr, n):
        # one structured-array copy instead of a dict per query (1000 queries: ~4 ms of getattr otherwise);
        # st[i]["pops"], iteration and len() work as they would on a list of dicts
        return np.frombuffer(arr, dtype=_STATS_DTYPE, count=n).copy()

    def query(self, sources, with_idx=False, want_ppr=True):
        src = np.ascontiguousarray(sources, dtype=np.int32)
        nq = src.size
        st = (QueryStats * max(1, nq))()
        out = np.zeros((nq, self.n), dtype=np.float64) if want_ppr else None
        self._chk(self._lib.fora_hip_query_batch(self._ctx, _p(src), nq, int(with_idx), _p(out), st))
        return out, self._stats(st, nq)

    def query_fix(self, sources, with_idx=False, want_residue=True):
        src = np.ascontiguousarray(sources, dtype=np.int32)
        nq = src.size
        st = (QueryStats * max(1, nq))()
        ppr = np.zeros((nq, self.n), dtype=np.uint64)
        res = np.zeros((nq, self.n), dtype=np.uint64) if want_residue else None
        self._chk(self._lib.fora_hip_query_batch_fix(self._ctx, _p(src), nq, int(with_idx), _p(ppr), _p(res), st))
        return ppr, res, self._stats(st, nq)

    def query_sparse(self, sources, with_idx=False, threshold=None, want_fix=False, device=False):
        """query() with the result kept sparse (fora_hip_query_sparse_batch + fora_hip_sparse_fetch): node v of row i is
        kept iff its fixed-point word is >= max(1, ceil(threshold * 2^62)); threshold=None: 1 / n.  Returns
        (row_ptr, ids, vals, stats, sparse_stats), with want_fix (row_ptr, ids, vals, fix, stats, sparse_stats): a CSR over
        the sources, ids ascending inside a row.  device=False: numpy arrays (int64, int32, float64, uint64).
        device=True: torch tensors on the context's GPU (fix as int64 bits), written there by the library; torch must have
        been imported before the library was loaded (one HIP runtime in the process)."""
        src = np.ascontiguousarray(sources, dtype=np.int32)
        nq = src.size
        st = (QueryStats * max(1, nq))()
        sp = SparseStats()
        row_ptr = np.zeros(nq + 1, dtype=np.int64)
        thr = 1.0 / self.n if threshold is None else float(threshold)
        self._chk(self._lib.fora_hip_query_sparse_batch(self._ctx, _p(src), nq, int(with_idx), thr, _p(row_ptr), st, C.byref(sp)))
        row_ptr, ids, vals, fix = self._sparse_result(row_ptr, int(sp.entries), want_fix, device, "query_sparse")
        out = (row_ptr, ids, vals) + ((fix,) if want_fix else ())
        return out + (self._stats(st, nq), sp.as_dict())

    def query_sparse_topk(self, sources, k, with_idx=False, threshold=None, want_fix=False, device=False):
        """query_sparse() with every row cut to its k largest entries on the GPU (fora_hip_query_sparse_topk_batch): word
        descending, ties by ascending id, the kept entries held in ascending id order.  k >= 1.  Returns what query_sparse
        returns plus the top-k stats: (row_ptr, ids, vals[, fix], stats, sparse_stats, topk_stats)."""
        src = np.ascontiguousarray(sources, dtype=np.int32)
        nq = src.size
        st = (QueryStats * max(1, nq))()
        sp, tk = SparseStats(), TopkStats()
        row_ptr = np.zeros(nq + 1, dtype=np.int64)
        thr = 1.0 / self.n if threshold is None else float(threshold)
        self._chk(self._lib.fora_hip_query_sparse_topk_batch(self._ctx, _p(src), nq, int(with_idx), thr, int(k), _p(row_ptr), st,
                                                             C.byref(sp), C.byref(tk)))
        row_ptr, ids, vals, fix = self._sparse_result(row_ptr, int(sp.entries), want_fix, device, "query_sparse_topk")
        out = (row_ptr, ids, vals) + ((fix,) if want_fix else ())
        return out + (self._stats(st, nq), sp.as_dict(), tk.as_dict())

    def _torch_device(self, who):
        """the context's GPU as a torch device, for who(device=True)"""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError(f"{who}(device=True): torch sees no GPU here.  torch and libfora_hip.so must share one "
                               "HIP runtime: import torch before the first Engine is created")
        return torch.device("cuda", self.device)

    def _held_outputs(self, specs, device, who):
        """The outputs of a held result, one per (length, numpy dtype, torch dtype name) of specs (None: not wanted): numpy
        zeros, or with device torch tensors on the context's GPU, the device synchronised once they are made.  Returns
        (arrays, pointers), None for an output that is not wanted."""
        if not device:
            arrs = [None if s is None else np.zeros(s[0], dtype=s[1]) for s in specs]
            return arrs, [_p(a) for a in arrs]
        import torch
        dev = self._torch_device(who)
        arrs = [None if s is None else torch.empty(s[0], dtype=getattr(torch, s[2]), device=dev) for s in specs]
        torch.cuda.synchronize(dev)  # (the allocator may hand out memory another stream still uses)
        return arrs, [None if a is None else a.data_ptr() for a in arrs]

    def _sparse_result(self, row_ptr, e, want_fix, device, who):
        """The held sparse result of e entries through fora_hip_sparse_fetch: (row_ptr, ids, vals, fix or None) as numpy
        arrays, or with device as torch tensors on the context's GPU."""
        specs = [(e, np.int32, "int32"), (e, np.float64, "float64"), (e, np.uint64, "int64") if want_fix else None]
        (ids, vals, fix), ptrs = self._held_outputs(specs, device, who)
        self._chk(self._lib.fora_hip_sparse_fetch(self._ctx, *ptrs, e))
        if device:
            import torch
            row_ptr = torch.from_numpy(row_ptr).to(ids.device)
        return row_ptr, ids, vals, fix

    def sparse_fetch(self, ids=None, vals=None, fix=None, cap=0):
        """fora_hip_sparse_fetch into caller-made numpy arrays (any of them None): the held result, again."""
        self._chk(self._lib.fora_hip_sparse_fetch(self._ctx, _p(ids), _p(vals), _p(fix), int(cap)))

    def sparse_clear(self):
        self._chk(self._lib.fora_hip_sparse_clear(self._ctx))

    # ---- the row store (the ROW STORE contract of include/fora_hip.h)
    def store_put(self, row_ptr, append=False):
        """The held sparse result into the store (fora_hip_store_put), replacing it or, with append, behind its rows.
        row_ptr: as the sparse call returned it.  Returns the stats dict."""
        rp, nq, _ = self._row_ptr(row_ptr)
        st = StoreStats()
        self._chk(self._lib.fora_hip_store_put(self._ctx, _p(rp), nq, int(bool(append)), C.byref(st)))
        return st.as_dict()

    def _store_array(self, x, entries, np_dtype, name):
        """(pointer, on_device, keep-alive) of the ids / fix argument of store_load: `entries` elements, a numpy array or a
        one-dimensional torch tensor on the context's GPU (fix as uint64 words, or the same bits as int64)"""
        if self._is_torch(x):
            import torch
            want = (torch.int32,) if np_dtype == np.int32 else (torch.int64,) + ((torch.uint64,) if hasattr(torch, "uint64") else ())
            if not x.is_cuda or x.device.index != self.device:
                raise ValueError(f"a torch {name} must live on the context's GPU")
            if x.dtype not in want or x.dim() != 1 or x.shape[0] != entries:
                raise ValueError(f"{name} must hold one {np.dtype(np_dtype).name} per entry")
            v = x.detach()
            if entries > 1 and v.stride(0) != 1:
                v = v.contiguous()
            return C.c_void_p(v.data_ptr()), True, v
        a = np.asarray(x)
        if a.dtype == np.int64 and np_dtype == np.uint64:
            a = a.view(np.uint64)
        if a.dtype != np_dtype or a.ndim != 1 or a.shape[0] != entries:
            raise ValueError(f"{name} must hold one {np.dtype(np_dtype).name} per entry")
        a = np.ascontiguousarray(a)
        return _p(a), False, a

    def store_load(self, row_ptr, ids, fix, append=False):
        """The caller's rows into the store (fora_hip_store_load): row_ptr [nrows + 1] (host), ids (int32) and fix (uint64
        words; int64 bits are taken as they are) with row_ptr[-1] entries each -- numpy arrays, or torch tensors on the
        context's GPU, which the device reads in place (a slice of a larger tensor is fine).  Every id is checked on the GPU:
        inside [0, n) and strictly ascending inside a row.  Returns the stats dict."""
        rp, nrows, e = self._row_ptr(row_ptr)
        if rp.ndim != 1 or rp.size < 1:
            raise ValueError("row_ptr must hold nrows + 1 entries")
        e = max(e, 0)
        iptr, i_dev, _ki = self._store_array(ids, e, np.int32, "ids")
        fptr, f_dev, _kf = self._store_array(fix, e, np.uint64, "fix")
        if i_dev or f_dev:
            import torch
            torch.cuda.synchronize(torch.device("cuda", self.device))  # (the tensors may have been written on another stream)
        st = StoreStats()
        self._chk(self._lib.fora_hip_store_load(self._ctx, _p(rp), nrows, iptr, fptr, int(bool(append)), C.byref(st)))
        return st.as_dict()

    def store_take(self, rows):
        """Rows `rows` of the store, in that order, become the held sparse result (fora_hip_store_take): one copy on the GPU,
        no query.  Returns (row_ptr, stats): the row_ptr every call on the held rows takes (sparse_propagate, sparse_attention,
        torch_ops ...); sparse_fetch copies the rows out."""
        r = self._row_ptr(rows)[0].reshape(-1)
        row_ptr = np.zeros(r.size + 1, dtype=np.int64)
        st = StoreStats()
        self._chk(self._lib.fora_hip_store_take(self._ctx, _p(r), r.size, _p(row_ptr), C.byref(st)))
        return row_ptr, st.as_dict()

    def store_info(self):
        """{rows, entries, max_row} of the store (fora_hip_store_info); zeros without one"""
        rows, entries, max_row = C.c_int64(0), C.c_uint64(0), C.c_uint64(0)
        self._chk(self._lib.fora_hip_store_info(self._ctx, C.byref(rows), C.byref(entries), C.byref(max_row)))
        return {"rows": rows.value, "entries": entries.value, "max_row": max_row.value}

    def store_clear(self):
        self._chk(self._lib.fora_hip_store_clear(self._ctx))

    # ---- the held result over its own columns (the COLUMNS contract of include/fora_hip.h)
    @property
    def held_cols(self):
        """The columns of the calls on the held rows (the option "sparse_cols"): the held result's own nc after
        sparse_compact, the graph's n otherwise."""
        return self.get_option("sparse_cols")

    def sparse_compact(self, row_ptr, device=False):
        """The held sparse result re-expressed over its own columns (fora_hip_sparse_compact): every held id becomes its rank
        in cols, the ascending array of the distinct node ids among the held entries, and from here on every call on the held
        rows takes operands with len(cols) rows in place of n (X[cols] for an X over the nodes) and returns column-sided
        outputs of that many rows -- the n_id of a sampled mini-batch.  row_ptr: as the sparse call or store_take returned
        it.  Returns (cols, stats dict): cols a numpy int32 array, or with device=True a torch int32 tensor on the context's
        GPU.  Ends with the held result; a second compaction of the same result is refused."""
        rp, nq, _ = self._row_ptr(row_ptr)
        nc, st = C.c_int64(0), ColsStats()
        if device:
            self._torch_device("sparse_compact")  # (refused before anything is compacted)
        self._chk(self._lib.fora_hip_sparse_compact(self._ctx, _p(rp), nq, C.byref(nc), C.byref(st)))
        (cols,), (ptr,) = self._held_outputs([(nc.value, np.int32, "int32")], device, "sparse_compact")
        self._chk(self._lib.fora_hip_sparse_cols_fetch(self._ctx, ptr if nc.value else None, nc.value))
        return cols, st.as_dict()

    def store_take_compact(self, rows, device=False):
        """store_take, then sparse_compact: rows `rows` of the store become the held result over their own columns.  Returns
        (row_ptr, cols, stats dict of the compaction)."""
        row_ptr, _ = self.store_take(rows)
        cols, st = self.sparse_compact(row_ptr, device=device)
        return row_ptr, cols, st

    # ---- the induced subgraph of the compacted held result (the SUBGRAPH contract of include/fora_hip_ext.h)
    def sparse_subgraph(self, row_ptr, want_eid=False, device=False):
        """The subgraph the graph induces on cols, the columns of the compacted held result (fora_hip_sparse_subgraph): a CSR
        over len(cols) rows in local ids -- row j holds the out-edges of node cols[j] whose target is in cols, in the graph's
        own order, multi-edges and self-loops as they stand.  row_ptr: as the sparse call or store_take returned it (the
        result must have been compacted: sparse_compact, store_take_compact).  Returns (sub_ptr, sub_col, sub_eid, stats
        dict): sub_ptr int64 [len(cols) + 1], sub_col int32 the targets' ranks in cols, sub_eid int64 the edges' places in
        the graph's col array (None unless want_eid) -- numpy arrays, or with device=True torch tensors on the context's GPU;
        stats: edges, scanned (the out-degrees of cols, added up: the edges read), sub_ms (device time of the kernels).
        subgraph_edge_index makes the COO pair of it.  Ends with the held result."""
        rp, nq, _ = self._row_ptr(row_ptr)
        edges, scanned, ms = C.c_int64(0), C.c_uint64(0), C.c_double(0)
        if device:
            self._torch_device("sparse_subgraph")  # (refused before anything is built)
        self._chk(self._lib.fora_hip_sparse_subgraph(self._ctx, _p(rp), nq, C.byref(edges), C.byref(scanned), C.byref(ms)))
        e, nc = edges.value, self.held_cols
        specs = [(nc + 1, np.int64, "int64"), (e, np.int32, "int32"), (e, np.int64, "int64") if want_eid else None]
        (sub_ptr, sub_col, sub_eid), ptrs = self._held_outputs(specs, device, "sparse_subgraph")
        self._chk(self._lib.fora_hip_sparse_subgraph_fetch(self._ctx, *ptrs, e))
        return sub_ptr, sub_col, sub_eid, {"edges": e, "scanned": scanned.value, "sub_ms": ms.value}

    def store_take_subgraph(self, rows, want_eid=False, device=False):
        """store_take, sparse_compact, sparse_subgraph: rows `rows` of the store become the held result over their own
        columns, with the graph's edges among those columns.  Returns (row_ptr, cols, sub_ptr, sub_col, sub_eid or None,
        stats dict of the subgraph)."""
        row_ptr, cols, _ = self.store_take_compact(rows, device=device)
        sub_ptr, sub_col, sub_eid, st = self.sparse_subgraph(row_ptr, want_eid=want_eid, device=device)
        return row_ptr, cols, sub_ptr, sub_col, sub_eid, st

    # ---- message passing on the held subgraph (the SUBGRAPH PRODUCTS contract of include/fora_hip_gnn.h)
    def _subgraph_product(self, fn, who, X, values, mean, want32, want64, out32, out64, bf16):
        nc, edges = self.held_cols, self.get_option("sub_edges")
        if edges < 0:
            raise ForaError(-1, f"{who}: no subgraph is held (sparse_subgraph first)")
        if mean and values is not None:
            raise ForaError(-1, f"{who}: mean and values exclude each other (pass 1 / count as values)")
        xptr, xtype, d, ldx, on_dev, _keep = self._prop_feat(X, bf16, rows=nc, name="X", shape="[nc, d] (nc: the held columns)")
        vptr, vtype, _vkeep = None, PROP_F32, None
        if values is not None:
            vptr, vtype, _, _vkeep = self._entry_operand(values, edges, "values", beside=on_dev)
            if edges == 0:
                vptr = None
        out32, out64, p32, p64, ldo = self._prop_outputs(nc, d, on_dev, want32, want64, out32, out64)
        info, ms = (C.c_int64 * 4)(), (C.c_double * 3)()
        flags = SUB_MEAN if mean else 0
        self._chk(fn(self._ctx, xptr, xtype, d, ldx, flags, vptr, vtype, p32, p64, ldo, info, ms))
        return out32, out64, {"edges": edges, "built": int(info[0]), "long_rows": int(info[1]), "chunks": int(info[2]), "x_on_device": int(info[3]),
                              "transpose_ms": ms[0], "short_ms": ms[1], "long_ms": ms[2]}

    def subgraph_propagate(self, X, values=None, mean=False, want32=True, want64=False, out32=None, out64=None, bf16=False):
        """out = A_S x X over the held subgraph (fora_hip_subgraph_propagate, the SUBGRAPH PRODUCTS contract of
        include/fora_hip_gnn.h): out[j] = sum over the edges e of row j of sparse_subgraph's CSR, in the order of sub_col, of
        w_e * X[sub_col[e]] -- the aggregation over the out-neighbours of cols[j] inside the batch, multi-edges as often as
        they stand, every bit defined.  X: [nc, d] (nc = held_cols), with the conventions of sparse_propagate's feat: a numpy
        float32 / float16 array, uint16 or uint8 codes with bf16=True / "bf16" / "e4m3" / "e5m2", or a torch tensor on the
        context's GPU (a column slice is read in place).  values: one float32 or float64 per edge of the subgraph in the
        order of sub_col (None: every weight 1.0) -- numpy, or a torch tensor beside a torch X.  mean: every output row
        divided by the number of its edges (a row without edges is 0); not together with values.  Returns (out32 or None,
        out64 or None, stats dict): [nc, d], torch tensors with a torch X, numpy arrays otherwise; out32 / out64:
        caller-made outputs as for sparse_propagate.  stats: edges, built (this call built the transposition), long_rows
        (output rows longer than the option "sub_short"), chunks of their path, x_on_device, and the device times
        transpose_ms, short_ms, long_ms."""
        return self._subgraph_product(self._lib.fora_hip_subgraph_propagate, "subgraph_propagate", X, values, mean, want32, want64, out32, out64, bf16)

    def subgraph_propagate_t(self, G, values=None, mean=False, want32=True, want64=False, out32=None, out64=None, bf16=False):
        """out = A_S^T x G over the held subgraph (fora_hip_subgraph_propagate_t): out[v] = sum over the edges e with
        sub_col[e] == v, in ascending e, of w_e * G[row of e] -- the aggregation over in-neighbours, and the gradient of
        subgraph_propagate with respect to X when G is the gradient with respect to its output.  values is still indexed by
        the edge's place in sub_col; mean divides by a column's number of edges.  Operands, outputs and stats as for
        subgraph_propagate; the first transposed call on a held subgraph builds its transposition (stats["built"] == 1)."""
        return self._subgraph_product(self._lib.fora_hip_subgraph_propagate_t, "subgraph_propagate_t", G, values, mean, want32, want64, out32, out64, bf16)

    def subgraph_degrees(self, transposed=False, device=False):
        """The number of edges of every row of the held subgraph (transposed: of every column; this builds the transposition
        if it is not there): int64 [nc], numpy or with device=True a torch tensor -- the counts FORA_SUB_MEAN divides by."""
        nc, edges = self.held_cols, self.get_option("sub_edges")
        if edges < 0:
            raise ForaError(-1, "subgraph_degrees: no subgraph is held (sparse_subgraph first)")
        (ptr,), (p,) = self._held_outputs([(nc + 1, np.int64, "int64")], device, "subgraph_degrees")
        fetch = self._lib.fora_hip_subgraph_transpose_fetch if transposed else self._lib.fora_hip_sparse_subgraph_fetch
        self._chk(fetch(self._ctx, p, None, None, edges))
        return ptr[1:] - ptr[:-1]

    def subgraph_transpose_fetch(self, device=False):
        """The transposition of the held subgraph (fora_hip_subgraph_transpose_fetch), built if it is not there: (in_ptr int64
        [nc + 1], in_row int32, in_pos int64 [edges]) -- column by column the local row every entry came from and the edge's
        place in sub_col, ascending inside a column.  numpy arrays, or with device=True torch tensors on the context's GPU."""
        nc, edges = self.held_cols, self.get_option("sub_edges")
        if edges < 0:
            raise ForaError(-1, "subgraph_transpose_fetch: no subgraph is held (sparse_subgraph first)")
        specs = [(nc + 1, np.int64, "int64"), (edges, np.int32, "int32"), (edges, np.int64, "int64")]
        (in_ptr, in_row, in_pos), ptrs = self._held_outputs(specs, device, "subgraph_transpose_fetch")
        self._chk(self._lib.fora_hip_subgraph_transpose_fetch(self._ctx, *ptrs, edges))
        return in_ptr, in_row, in_pos

    # ---- feature propagation (the PROPAGATE contract of include/fora_hip.h)
    @staticmethod
    def _is_torch(x):
        return type(x).__module__.split(".")[0] == "torch"

    def _row_ptr(self, row_ptr):
        """(rp, nq, entries) of the row_ptr argument of the calls on the held rows: a host int64 array of nq + 1 offsets, from
        a numpy array or a torch tensor"""
        if self._is_torch(row_ptr):
            row_ptr = row_ptr.cpu().numpy()
        rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
        return rp, rp.size - 1, int(rp.reshape(-1)[-1]) if rp.size else 0

    def _prop_feat(self, feat, bf16, rows=None, name="feat", shape=None):
        """(pointer, feat_type, d, ldf, on_device, keep-alive) of the feat argument of sparse_propagate ([n, d]; n: the held
        columns, held_cols), or with rows / name of the grad argument of sparse_propagate_t ([nq, d]; shape: how the
        message names another shape).  The element type comes from a torch tensor's dtype (float32, bfloat16, float16,
        float8_e4m3fn, float8_e5m2) and from a numpy array's (float32, float16); the codes of bf16 and FP8 have no numpy dtype
        and come as uint16 with the operand's keyword (bf16=, a_bf16=, q_bf16= ...) True or "bf16", as uint8 with "e4m3" or
        "e5m2" -- the calls' docstrings say "bf16=True" for short.  Every other dtype is a ValueError."""
        shape = shape or ("[n, d] (n: the held columns)" if rows is None else "[nq, d]")
        rows = self.held_cols if rows is None else rows
        if self._is_torch(feat):
            import torch
            if not feat.is_cuda or feat.device.index != self.device:
                raise ValueError(f"a torch {name} must live on the context's GPU")
            types = {torch.float32: PROP_F32, torch.bfloat16: PROP_BF16, torch.float16: PROP_F16, torch.float8_e4m3fn: PROP_E4M3,
                     torch.float8_e5m2: PROP_E5M2}
            if feat.dtype not in types:
                raise ValueError(f"a torch {name} must be float32, bfloat16, float16, float8_e4m3fn or float8_e5m2")
            if feat.dim() != 2 or feat.shape[0] != rows or (feat.shape[1] > 1 and feat.stride(1) != 1):
                raise ValueError(f"{name} must be {shape} with a column stride of one element")
            ldf = feat.stride(0) if feat.shape[0] > 1 else feat.shape[1]
            return C.c_void_p(feat.data_ptr()), types[feat.dtype], int(feat.shape[1]), int(ldf), True, feat
        a = np.asarray(feat)
        # the keyword says what the codes of an integer array are: True or "bf16" for uint16, "e4m3" or "e5m2" for uint8
        if isinstance(bf16, str):
            if bf16 not in ("bf16", "e4m3", "e5m2"):
                raise ValueError(f'{name}: the element type "{bf16}" is not "bf16", "e4m3" or "e5m2"')
            ftype, want = {"bf16": (PROP_BF16, np.uint16), "e4m3": (PROP_E4M3, np.uint8), "e5m2": (PROP_E5M2, np.uint8)}[bf16]
        elif bf16:
            ftype, want = PROP_BF16, np.uint16
        elif a.dtype == np.float16:
            ftype, want = PROP_F16, np.float16
        else:
            ftype, want = PROP_F32, np.float32
        if a.dtype != want:
            raise ValueError(f'a numpy {name} must be float32 or float16, or uint16 with bf16=True, or uint8 with "e4m3" or "e5m2" in its place')
        if a.ndim != 2 or a.shape[0] != rows:
            raise ValueError(f"{name} must be {shape}")
        it = a.itemsize
        if a.shape[0] == 0:                     # (no rows -- a compacted result without columns: nothing is read, and numpy's strides say nothing)
            a = np.zeros((0, a.shape[1]), dtype=a.dtype)
        elif (a.shape[1] > 1 and a.strides[1] != it) or (a.shape[0] > 1 and (a.strides[0] % it or a.strides[0] < a.shape[1] * it)):
            raise ValueError(f"{name}: a column stride other than one element (or rows that overlap) is not supported")
        ldf = a.strides[0] // it if a.shape[0] > 1 else a.shape[1]
        return _p(a), ftype, int(a.shape[1]), int(ldf), False, a

    def _prop_out(self, out, nq, d, dtype, on_device, name):
        """(pointer, ldo, array) of a caller-made output ([nq, d], row stride = ldo) -- it must live where feat lives"""
        if self._is_torch(out) != on_device:
            raise ValueError(f"{name}: a torch tensor with a torch feat, a numpy array otherwise")
        if on_device:
            ok = out.dim() == 2 and tuple(out.shape) == (nq, d) and (d == 1 or out.stride(1) == 1) and out.is_cuda and out.device.index == self.device
            ldo = out.stride(0) if nq > 1 else d
            ptr = C.c_void_p(out.data_ptr())
            ok = ok and out.dtype == dtype
        else:
            ok = out.ndim == 2 and out.shape == (nq, d) and out.dtype == dtype
            ok = ok and (nq == 0 or ((d == 1 or out.strides[1] == out.itemsize) and out.strides[0] % out.itemsize == 0))  # (no rows: numpy's strides say nothing)
            ldo = out.strides[0] // out.itemsize if nq > 1 else d
            ptr = _p(out)
        if not ok or ldo < d:
            raise ValueError(f"{name} must be [nq, d] of the output's type with a column stride of one element")
        return ptr, int(ldo)

    def sparse_propagate(self, row_ptr, feat, normalize=False, want32=True, want64=False, bf16=False, out32=None, out64=None, values=None):
        """out = (held sparse rows) x feat (fora_hip_sparse_propagate, the PROPAGATE contract of include/fora_hip.h), on the held
        result of query_sparse / query_seeds_sparse: out[i, c] = sum over the entries of row i of val * feat[id, c] in the
        contract's fixed order, every bit defined.  row_ptr: as the sparse call returned it.  feat: a numpy float32 array
        [n, d] (the row stride becomes ldf; a column stride other than one element is rejected), a numpy uint16 array with
        bf16=True, or a torch tensor on the context's GPU (float32 or bfloat16, any row stride: a column slice of a wider
        tensor is read in place).  The narrow types (float16, FP8 E4M3 / E5M2), here and in every call below: _prop_feat.  normalize: every row divided by the sum of its kept values.  Returns
        (out32 or None, out64 or None, stats dict): float32 / float64 [nq, d]; torch tensors on the device with a torch
        feat, numpy arrays otherwise.  out32 / out64: caller-made outputs to fill instead (their row stride is ldo; columns
        past d are left alone), both with the same row stride.  values (fora_hip_sparse_propagate_vals, PROPAGATE WITH
        VALUES): one float32 or float64 per held entry, in held order, used as the weights in place of the held values --
        numpy, or a torch tensor on the GPU beside a torch feat; not together with normalize."""
        rp, nq, e = self._row_ptr(row_ptr)
        fptr, ftype, d, ldf, on_dev, _keep = self._prop_feat(feat, bf16)
        fn, vals = self._lib.fora_hip_sparse_propagate, ()
        if values is not None:
            vptr, vtype, _, _vkeep = self._entry_operand(values, e, "values", beside=on_dev)
            fn, vals = self._lib.fora_hip_sparse_propagate_vals, (vptr, vtype)
        out32, out64, p32, p64, ldo = self._prop_outputs(nq, d, on_dev, want32, want64, out32, out64)
        ps = PropStats()
        self._chk(fn(self._ctx, _p(rp), nq, fptr, ftype, d, ldf, PROP_NORMALIZE if normalize else 0, *vals, p32, p64, ldo, C.byref(ps)))
        return out32, out64, ps.as_dict()

    def _prop_outputs(self, rows, d, on_dev, want32, want64, out32, out64):
        """the outputs of sparse_propagate / sparse_propagate_t ([rows, d]): made here where the caller brought none, on the
        device (after a device synchronise) with on_dev.  Returns (out32, out64, pointer32, pointer64, ldo)."""
        if on_dev:
            import torch
            dev = torch.device("cuda", self.device)
            if out32 is None and want32:
                out32 = torch.empty((rows, d), dtype=torch.float32, device=dev)
            if out64 is None and want64:
                out64 = torch.empty((rows, d), dtype=torch.float64, device=dev)
            t32, t64 = torch.float32, torch.float64
            torch.cuda.synchronize(dev)  # (feat may have been written, and the allocator may hand out memory, on another stream)
        else:
            if out32 is None and want32:
                out32 = np.zeros((rows, d), dtype=np.float32)
            if out64 is None and want64:
                out64 = np.zeros((rows, d), dtype=np.float64)
            t32, t64 = np.float32, np.float64
        p32 = p64 = None
        ldo = d
        if out32 is not None:
            p32, ldo = self._prop_out(out32, rows, d, t32, on_dev, "out32")
        if out64 is not None:
            p64, ldo64 = self._prop_out(out64, rows, d, t64, on_dev, "out64")
            if out32 is not None and ldo64 != ldo:
                raise ValueError("out32 and out64 must have the same row stride in elements")
            ldo = ldo64
        return out32, out64, p32, p64, ldo

    def sparse_propagate_t(self, row_ptr, grad, normalize=False, want32=True, want64=False, bf16=False, out32=None, out64=None, values=None):
        """out = (held sparse rows)^T x grad (fora_hip_sparse_propagate_t, the PROPAGATE, TRANSPOSED contract of
        include/fora_hip.h): out[v, c] = sum over the held entries whose id is v, by ascending row, of val * grad[row, c] --
        the gradient of a loss with respect to the feat of sparse_propagate when grad is its gradient with respect to the
        output.  grad: [nq, d], a numpy float32 array (uint16 with bf16=True) or a torch tensor on the context's GPU, with the
        conventions of sparse_propagate's feat.  normalize: every value divided by the sum of its row's kept values (the
        adjoint of sparse_propagate(normalize=True)).  Returns (out32 or None, out64 or None, stats dict): [n, d], torch
        tensors on the device with a torch grad, numpy arrays otherwise.  The first call on a held result builds its
        transposition (stats["built"] == 1), later calls reuse it.  values (fora_hip_sparse_propagate_t_vals): as for
        sparse_propagate, one element per held entry in HELD order."""
        rp, nq, e = self._row_ptr(row_ptr)
        gptr, gtype, d, ldg, on_dev, _keep = self._prop_feat(grad, bf16, rows=nq, name="grad")
        fn, vals = self._lib.fora_hip_sparse_propagate_t, ()
        if values is not None:
            vptr, vtype, _, _vkeep = self._entry_operand(values, e, "values", beside=on_dev)
            fn, vals = self._lib.fora_hip_sparse_propagate_t_vals, (vptr, vtype)
        out32, out64, p32, p64, ldo = self._prop_outputs(self.held_cols, d, on_dev, want32, want64, out32, out64)
        ps = PropTStats()
        self._chk(fn(self._ctx, _p(rp), nq, gptr, gtype, d, ldg, PROP_NORMALIZE if normalize else 0, *vals, p32, p64, ldo, C.byref(ps)))
        return out32, out64, ps.as_dict()

    def sparse_sddmm(self, row_ptr, a, b, want32=True, want64=False, out32=None, out64=None, a_bf16=False, b_bf16=False):
        """scores[e] = <a[row of e], b[id of e]> for every held entry e (fora_hip_sparse_sddmm, the SCORES (SDDMM) contract of
        include/fora_hip.h), in the contract's fixed order, every bit defined.  a: [nq, d], b: [n, d], each a numpy float32
        array (uint16 with a_bf16 / b_bf16) or a torch tensor on the context's GPU (float32 or bfloat16), with the stride
        conventions of sparse_propagate's feat; the two may differ in type and in where they live.  Returns
        (out32 or None, out64 or None, stats dict): float32 / float64 [entries], torch tensors on the device when a or b is
        a torch tensor, numpy arrays otherwise; out32 / out64: caller-made contiguous outputs of at least `entries`
        elements to fill instead, each a numpy array or a torch tensor on the GPU."""
        rp, nq, e = self._row_ptr(row_ptr)
        aptr, atype, d, lda, a_dev, _ka = self._prop_feat(a, a_bf16, rows=nq, name="a")
        bptr, btype, db, ldb, b_dev, _kb = self._prop_feat(b, b_bf16, name="b")
        if db != d:
            raise ValueError("a and b must have the same number of columns")
        out32, out64, p32, p64, cap = self._entry_outputs(e, a_dev or b_dev, want32, want64, out32, out64)
        st = SddmmStats()
        self._chk(self._lib.fora_hip_sparse_sddmm(self._ctx, _p(rp), nq, aptr, atype, lda, bptr, btype, ldb, d, p32, p64, cap, C.byref(st)))
        return out32, out64, st.as_dict()

    def _entry_outputs(self, e, on_dev, want32, want64, out32, out64):
        """the per-entry outputs of sparse_sddmm / sparse_softmax ([entries]): made here where the caller brought none, on the
        device (and after a device synchronise) with on_dev.  Returns (out32, out64, pointer32, pointer64, cap)."""
        if on_dev:
            import torch
            dev = torch.device("cuda", self.device)
            mk = lambda bits: torch.empty(e, dtype=torch.float32 if bits == 32 else torch.float64, device=dev)
        else:
            mk = lambda bits: np.zeros(e, dtype=np.float32 if bits == 32 else np.float64)
        if out32 is None and want32:
            out32 = mk(32)
        if out64 is None and want64:
            out64 = mk(64)
        ptrs, cap = [], None
        for o, bits, name in ((out32, 32, "out32"), (out64, 64, "out64")):
            if o is None:
                ptrs.append(None)
                continue
            if self._is_torch(o):                        # (an output lives where its caller made it, whatever the operands do)
                import torch
                dt = torch.float32 if bits == 32 else torch.float64
                ok = o.dim() == 1 and o.dtype == dt and o.is_cuda and o.device.index == self.device and (o.numel() < 2 or o.stride(0) == 1)
                ptrs.append(C.c_void_p(o.data_ptr()))
                cnt = o.numel()
            else:
                ok = o.ndim == 1 and o.dtype == (np.float32 if bits == 32 else np.float64) and (o.size < 2 or o.strides[0] == o.itemsize)
                ptrs.append(_p(o))
                cnt = o.size
            if not ok:
                raise ValueError(f"{name} must be a contiguous one-dimensional array of the output's type")
            cap = cnt if cap is None else min(cap, cnt)
        if on_dev:
            torch.cuda.synchronize(dev)  # (the operands may have been written, and the allocator may hand out memory, on another stream)
        return out32, out64, ptrs[0], ptrs[1], cap or 0

    def _entry_operand(self, x, entries, name, beside=None):
        """(pointer, element type, on_device, keep-alive) of a per-entry input -- the scores / y / grad of sparse_softmax and
        sparse_softmax_bwd, the values of sparse_propagate and sparse_propagate_t: one float32 or float64 per held entry, a
        numpy array or a torch tensor on the context's GPU.  beside (the values only): whether the feat / grad beside them is
        a torch tensor -- torch values need one: the call synchronises the device once, for all its operands."""
        if self._is_torch(x):
            import torch
            if beside is False:
                raise ValueError(f"torch {name} go with a torch feat / grad")
            if not x.is_cuda or x.device.index != self.device:
                raise ValueError(f"{'torch' if beside else 'a torch'} {name} must live on the context's GPU")
            if x.dtype not in (torch.float32, torch.float64):
                raise ValueError(f"{name} must be float32 or float64")
            if x.dim() != 1 or x.shape[0] != entries:
                raise ValueError(f"{name} must hold one element per held entry")
            v = x.detach()
            if entries > 1 and v.stride(0) != 1:
                v = v.contiguous()
            return C.c_void_p(v.data_ptr()), (PROP_F64 if v.dtype == torch.float64 else PROP_F32), True, v
        a = np.asarray(x)
        if a.dtype not in (np.float32, np.float64):
            raise ValueError(f"{name} must be float32 or float64")
        if a.ndim != 1 or a.shape[0] != entries:
            raise ValueError(f"{name} must hold one element per held entry")
        a = np.ascontiguousarray(a)
        return _p(a), (PROP_F64 if a.dtype == np.float64 else PROP_F32), False, a

    def sparse_softmax(self, row_ptr, scores, scale=1.0, want32=True, want64=False, out32=None, out64=None):
        """y[e] = softmax inside its held row of scores[e] * scale (fora_hip_sparse_softmax, the ROW SOFTMAX contract of
        include/fora_hip.h): the row's maximum subtracted, the contract's exp_def, the row sum in its fixed order, one
        division -- every bit defined.  scores: one float32 or float64 per held entry in held order, a numpy array or a torch
        tensor on the context's GPU.  A row with a NaN, with +inf, or of -inf only becomes NaN (stats["nan_rows"]).  Returns
        (out32 or None, out64 or None, stats dict): [entries], torch tensors on the device when scores is one, numpy arrays
        otherwise; out32 / out64: caller-made contiguous outputs of at least `entries` elements, as for sparse_sddmm."""
        rp, nq, e = self._row_ptr(row_ptr)
        sptr, stype, on_dev, _keep = self._entry_operand(scores, e, "scores")
        out32, out64, p32, p64, cap = self._entry_outputs(e, on_dev, want32, want64, out32, out64)
        st = SoftmaxStats()
        self._chk(self._lib.fora_hip_sparse_softmax(self._ctx, _p(rp), nq, sptr, stype, float(scale), p32, p64, cap, C.byref(st)))
        return out32, out64, st.as_dict()

    def sparse_softmax_bwd(self, row_ptr, y, grad, scale=1.0, want32=True, want64=False, out32=None, out64=None):
        """dx[e] = ((grad[e] - D) * y[e]) * scale with D = the row's sum of y * grad in the contract's order
        (fora_hip_sparse_softmax_bwd): the gradient of sparse_softmax with respect to scores, y its output and scale its
        scale.  y and grad: float32 or float64 each, numpy or torch on the GPU; outputs as for sparse_softmax (torch when
        either input is)."""
        rp, nq, e = self._row_ptr(row_ptr)
        yptr, ytype, y_dev, _ky = self._entry_operand(y, e, "y")
        gptr, gtype, g_dev, _kg = self._entry_operand(grad, e, "grad")
        out32, out64, p32, p64, cap = self._entry_outputs(e, y_dev or g_dev, want32, want64, out32, out64)
        st = SoftmaxStats()
        self._chk(self._lib.fora_hip_sparse_softmax_bwd(self._ctx, _p(rp), nq, yptr, ytype, gptr, gtype, float(scale),
                                                        p32, p64, cap, C.byref(st)))
        return out32, out64, st.as_dict()

    def sparse_attention(self, row_ptr, Q, K, V, heads=1, scale=None, want32=True, want64=False, want_y32=False, want_y64=False,
                         out32=None, out64=None, q_bf16=False, k_bf16=False, v_bf16=False):
        """out = softmax inside every held row of (scale * <Q[row], K[id]>) times V, head by head, in ONE call
        (fora_hip_sparse_attention, the ATTENTION contract of include/fora_hip.h): bit for bit sparse_sddmm (float64), then
        sparse_softmax, then sparse_propagate(values=...) on the column slices of the heads.  Q: [nq, heads * d], K:
        [n, heads * d], V: [n, heads * dv], each a numpy float32 array (uint16 with q_bf16 / k_bf16 / v_bf16) or a torch
        tensor on the context's GPU (float32 or bfloat16), with the stride conventions of sparse_propagate's feat.  scale:
        d ** -0.5 when None.  Returns (out32 or None, out64 or None, y32 or None, y64 or None, stats dict): out
        [nq, heads * dv], y (the probabilities, with want_y32 / want_y64) [heads, entries]; torch tensors on the device when
        an operand is a torch tensor, numpy arrays otherwise.  out32 / out64: caller-made outputs as for sparse_propagate.
        A (row, head) with a NaN score, a +inf, or -inf only is written as NaN (stats["nan_rows"])."""
        rp, nq, e = self._row_ptr(row_ptr)
        heads = int(heads)
        qptr, qtype, wq, ldq, q_dev, _kq = self._prop_feat(Q, q_bf16, rows=nq, name="Q")
        kptr, ktype, wk, ldk, k_dev, _kk = self._prop_feat(K, k_bf16, name="K")
        vptr, vtype, wv, ldv, v_dev, _kv = self._prop_feat(V, v_bf16, name="V")
        if heads < 1 or wq % heads or wv % heads:
            raise ValueError("heads must be at least 1 and divide the columns of Q and of V")
        if wk != wq:
            raise ValueError("Q and K must have the same number of columns")
        d, dv = wq // heads, wv // heads
        on_dev = q_dev or k_dev or v_dev
        if on_dev and not (q_dev and k_dev and v_dev):
            raise ValueError("Q, K and V: all torch tensors on the GPU, or all numpy arrays")
        y32, y64, py32, py64, ycap = self._entry_outputs(heads * e, on_dev, want_y32, want_y64, None, None)
        out32, out64, p32, p64, ldo = self._prop_outputs(nq, wv, on_dev, want32, want64, out32, out64)
        st = AttnStats()
        sc = float(d) ** -0.5 if scale is None else float(scale)
        self._chk(self._lib.fora_hip_sparse_attention(self._ctx, _p(rp), nq, qptr, qtype, ldq, kptr, ktype, ldk, vptr, vtype, ldv, d, dv, heads, sc,
                                                      p32, p64, ldo, py32, py64, ycap, C.byref(st)))
        if y32 is not None:
            y32 = y32.reshape(heads, e)
        if y64 is not None:
            y64 = y64.reshape(heads, e)
        return out32, out64, y32, y64, st.as_dict()

    def sparse_attention_bwd(self, row_ptr, Q, K, V, G, y, heads=1, scale=None, want_dq=True, want_dk=True, want_dv=True, want32=True, want64=False,
                             q_bf16=False, k_bf16=False, v_bf16=False, g_bf16=False, dq32=None, dq64=None, dk32=None, dk64=None, dv32=None, dv64=None):
        """The gradients of sparse_attention with respect to Q, K and V for all heads in ONE call
        (fora_hip_sparse_attention_bwd, the ATTENTION, BACKWARD contract of include/fora_hip.h): bit for bit sparse_sddmm(G, V)
        (float64), sparse_softmax_bwd(y, .), sparse_propagate(K, values=ds), sparse_propagate_t(Q, values=ds) and
        sparse_propagate_t(G, values=y) on the column slices of the heads, nothing rounded to float32 in between.  Q, K, V:
        as for sparse_attention; G: [nq, heads * dv], the gradient of its output (float32, or uint16 with g_bf16, or a torch
        tensor); y: [heads, entries] float32 or float64, the probabilities the forward call returned.  All operands torch
        tensors on the context's GPU, or all numpy arrays.  want_dq / want_dk / want_dv: a gradient that is not wanted is
        not computed.  Returns (dq32, dq64, dk32, dk64, dv32, dv64, stats dict): dq [nq, heads * d], dk [n, heads * d], dv
        [n, heads * dv], None where not wanted; dq32 .. dv64: caller-made outputs to fill instead, as for sparse_propagate
        (the two of one gradient with the same row stride; a caller-made output makes its gradient wanted).  The first call on
        a held result builds its transposition (stats["built"] == 1) and plans the columns; later calls reuse both
        (stats["plan_cached"] == 1)."""
        rp, nq, e = self._row_ptr(row_ptr)
        heads = int(heads)
        qptr, qtype, wq, ldq, q_dev, _kq = self._prop_feat(Q, q_bf16, rows=nq, name="Q")
        kptr, ktype, wk, ldk, k_dev, _kk = self._prop_feat(K, k_bf16, name="K")
        vptr, vtype, wv, ldv, v_dev, _kv = self._prop_feat(V, v_bf16, name="V")
        gptr, gtype, wg, ldg, g_dev, _kg = self._prop_feat(G, g_bf16, rows=nq, name="G")
        if heads < 1 or wq % heads or wv % heads:
            raise ValueError("heads must be at least 1 and divide the columns of Q and of V")
        if wk != wq or wg != wv:
            raise ValueError("Q and K, and V and G, must have the same number of columns")
        d, dv = wq // heads, wv // heads
        on_dev = q_dev or k_dev or v_dev or g_dev or self._is_torch(y)
        if on_dev and not (q_dev and k_dev and v_dev and g_dev and self._is_torch(y)):
            raise ValueError("Q, K, V, G and y: all torch tensors on the GPU, or all numpy arrays")
        if tuple(y.shape) != (heads, e):
            raise ValueError("y must be [heads, entries]")
        yptr, ytype, _, _ky = self._entry_operand(y.reshape(heads * e), heads * e, "y")
        gr = AttnGrads()
        outs = []
        nc = self.held_cols
        for name, rows, w, want, o32, o64 in (("dq", nq, wq, want_dq, dq32, dq64), ("dk", nc, wq, want_dk, dk32, dk64), ("dv", nc, wv, want_dv, dv32, dv64)):
            want = want or o32 is not None or o64 is not None
            o32, o64, p32, p64, ld = self._prop_outputs(rows, w, on_dev, want and want32, want and want64, o32, o64) if want else (None, None, None, None, w)
            setattr(gr, name + "32", p32.value if p32 is not None else None)
            setattr(gr, name + "64", p64.value if p64 is not None else None)
            setattr(gr, "ld" + name, ld)
            outs += [o32, o64]
        st = AttnBwdStats()
        sc = float(d) ** -0.5 if scale is None else float(scale)
        self._chk(self._lib.fora_hip_sparse_attention_bwd(self._ctx, _p(rp), nq, qptr, qtype, ldq, kptr, ktype, ldk, vptr, vtype, ldv, gptr, gtype, ldg,
                                                          yptr, ytype, heads * e, d, dv, heads, sc, C.byref(gr), C.byref(st)))
        return (*outs, st.as_dict())

    def sparse_transpose_fetch(self, row_ptr, want_fix=False, device=False):
        """The transposition of the held sparse result (fora_hip_sparse_transpose_fetch): (col_ptr, rows, vals), with want_fix
        (col_ptr, rows, vals, fix) -- a CSR over the n nodes, column v listing the rows that keep v in ascending order.
        device=False: numpy arrays (int64, int32, float64, uint64); device=True: torch tensors on the context's GPU (fix as
        int64 bits), as for query_sparse."""
        rp, nq, e = self._row_ptr(row_ptr)
        specs = [(self.held_cols + 1, np.int64, "int64"), (e, np.int32, "int32"), (e, np.uint64, "int64") if want_fix else None,
                 (e, np.float64, "float64")]
        (col_ptr, rows, fix, vals), ptrs = self._held_outputs(specs, device, "sparse_transpose_fetch")
        self._chk(self._lib.fora_hip_sparse_transpose_fetch(self._ctx, _p(rp), nq, *ptrs, e))
        return (col_ptr, rows, vals) + ((fix,) if want_fix else ())

    def _propagate_chunks(self, total, chunk, feat, bf16, want32, want64, normalize, run):
        """the frame of propagate / propagate_seeds: run(i0, i1) leaves the held sparse result of rows [i0, i1) and returns
        its row_ptr; every chunk's product lands in its rows of one [total, d] output"""
        # (over the graph's n nodes, whatever is held now: run() replaces the held result, and a compacted state ends there)
        _, _, d, _, on_dev, _keep = self._prop_feat(feat, bf16, rows=self.n, shape="[n, d]")
        if on_dev:
            import torch
            dev = torch.device("cuda", self.device)
            out32 = torch.zeros((total, d), dtype=torch.float32, device=dev) if want32 else None
            out64 = torch.zeros((total, d), dtype=torch.float64, device=dev) if want64 else None
        else:
            out32 = np.zeros((total, d), dtype=np.float32) if want32 else None
            out64 = np.zeros((total, d), dtype=np.float64) if want64 else None
        step = total if not chunk or chunk <= 0 else int(chunk)
        props = []
        for i0 in range(0, total, max(step, 1)):
            i1 = min(total, i0 + step)
            rp = run(i0, i1)
            _, _, ps = self.sparse_propagate(rp, feat, normalize=normalize, bf16=bf16, want32=False, want64=False,
                                             out32=None if out32 is None else out32[i0:i1], out64=None if out64 is None else out64[i0:i1])
            props.append(ps)
        return out32, out64, props

    def propagate(self, sources, feat, with_idx=False, threshold=None, normalize=False, chunk=None, want32=True, want64=False, bf16=False,
                  topk=None):
        """query_sparse then sparse_propagate, per chunk of `chunk` sources (None: all at once), into one [nq, d] output:
        nothing sparse leaves the device.  REPLACES the held sparse result (the last chunk's rows stay held).  Returns a
        dict: out32 / out64 (as sparse_propagate), stats (the per-query stats), prop (one stats dict per chunk).
        topk=k: the rows are query_sparse_topk's (their k largest entries); None: the full thresholded rows."""
        src = np.ascontiguousarray(sources, dtype=np.int32)
        nq = src.size
        st = (QueryStats * max(1, nq))()
        thr = 1.0 / self.n if threshold is None else float(threshold)

        def run(i0, i1):
            rp = np.zeros(i1 - i0 + 1, dtype=np.int64)
            part = (QueryStats * (i1 - i0)).from_buffer(st, i0 * C.sizeof(QueryStats))
            if topk is None:
                self._chk(self._lib.fora_hip_query_sparse_batch(self._ctx, _p(src[i0:i1]), i1 - i0, int(with_idx), thr, _p(rp), part, None))
            else:
                self._chk(self._lib.fora_hip_query_sparse_topk_batch(self._ctx, _p(src[i0:i1]), i1 - i0, int(with_idx), thr, int(topk),
                                                                     _p(rp), part, None, None))
            return rp
        out32, out64, props = self._propagate_chunks(nq, chunk, feat, bf16, want32, want64, normalize, run)
        return {"out32": out32, "out64": out64, "stats": self._stats(st, nq), "prop": props}

    def propagate_seeds(self, sets, weights, feat, with_idx=False, threshold=None, normalize=False, chunk=None, want32=True, want64=False,
                        bf16=False, topk=None):
        """query_seeds_sparse then sparse_propagate, per chunk of `chunk` sets (None: all at once), into one [ns, d] output.
        sets / weights as for query_seeds.  REPLACES the held sparse result.  Returns a dict: out32 / out64, prop.
        topk=k: the rows are query_seeds_sparse_topk's; None: the full thresholded rows."""
        set_ptr, seeds, w = self._seed_sets(sets, weights)
        ns = set_ptr.size - 1
        thr = 1.0 / self.n if threshold is None else float(threshold)

        def run(i0, i1):
            rp = np.zeros(i1 - i0 + 1, dtype=np.int64)
            lo, hi = int(set_ptr[i0]), int(set_ptr[i1])
            sp_ = np.ascontiguousarray(set_ptr[i0:i1 + 1] - lo)
            sd_ = np.ascontiguousarray(seeds[lo:hi])
            w_ = None if w is None else np.ascontiguousarray(w[lo:hi])
            if topk is None:
                self._chk(self._lib.fora_hip_seeds_sparse_batch(self._ctx, _p(sp_), _p(sd_), _p(w_), i1 - i0, int(with_idx),
                                                                thr, _p(rp), None, None, None))
            else:
                self._chk(self._lib.fora_hip_seeds_sparse_topk_batch(self._ctx, _p(sp_), _p(sd_), _p(w_), i1 - i0, int(with_idx),
                                                                     thr, int(topk), _p(rp), None, None, None, None))
            return rp
        out32, out64, props = self._propagate_chunks(ns, chunk, feat, bf16, want32, want64, normalize, run)
        return {"out32": out32, "out64": out64, "prop": props}

    # ---- local clustering (the SWEEP CUT contract of include/fora_hip.h)
    def sweep(self, sources, with_idx=False, threshold=None, max_size=0, want_profile=False, device=False):
        """query() followed on the GPU by the sweep over ppr / degree of every row (fora_hip_sweep_batch): the support
        {v : word >= max(1, ceil(threshold * 2^62))} (threshold=None: 1 / n) in sweep order, the cut and the volume of every
        prefix of at most max_size nodes (0: all), and the prefix of least conductance.  Returns a dict: row_ptr (int64
        [nq + 1], prefix sums of the profile lengths), rows (a structured array: len, best, cut, vol, den, conductance),
        stats, sweep (a dict), and with want_profile ids / cut / vol (int32 / uint64 / uint64; device=True: torch tensors
        on the context's GPU, the u64 ones as int64 bits).  The best cluster of row i is
        ids[row_ptr[i] : row_ptr[i] + rows[i]["best"]]."""
        src = np.ascontiguousarray(sources, dtype=np.int32)
        nq = src.size
        st = (QueryStats * max(1, nq))()
        rows = (SweepRow * max(1, nq))()
        sw = SweepStats()
        row_ptr = np.zeros(nq + 1, dtype=np.int64)
        thr = 1.0 / self.n if threshold is None else float(threshold)
        self._chk(self._lib.fora_hip_sweep_batch(self._ctx, _p(src), nq, int(with_idx), thr, int(max_size), _p(row_ptr), rows, st,
                                                 C.byref(sw)))
        out = {"row_ptr": row_ptr, "rows": np.frombuffer(rows, dtype=_SWEEP_ROW_DTYPE, count=nq).copy(),
               "stats": self._stats(st, nq), "sweep": sw.as_dict()}
        if want_profile:
            out["ids"], out["cut"], out["vol"] = self.sweep_fetch(int(row_ptr[-1]), device=device)
        return out

    def sweep_fetch(self, entries, device=False):
        """The held profile, again (fora_hip_sweep_fetch): (ids, cut, vol) of `entries` entries each."""
        e = int(entries)
        specs = [(e, np.int32, "int32"), (e, np.uint64, "int64"), (e, np.uint64, "int64")]
        (ids, cut, vol), ptrs = self._held_outputs(specs, device, "sweep_fetch")
        self._chk(self._lib.fora_hip_sweep_fetch(self._ctx, *ptrs, e))
        return ids, cut, vol

    def sweep_clear(self):
        self._chk(self._lib.fora_hip_sweep_clear(self._ctx))

    # ---- the TEST ENTRY POINTS of include/fora_hip.h: Engine(lib=TEST_LIB) only
    def _test_entry(self, name):
        if not hasattr(self._lib, name):
            raise ForaError(-1, f"{name} is in libfora_hip_test.so only: Engine(lib=capi.TEST_LIB)")
        return getattr(self._lib, name)

    def test_sweep_rows(self, rows_fix, threshold=None, max_size=0, want_profile=True):
        """sweep() over caller-made rows ([nq, n] fixed-point words) instead of a query's (fora_hip_test_sweep_rows): the
        same dict, without "stats"."""
        fix = np.ascontiguousarray(rows_fix, dtype=np.uint64)
        if fix.ndim != 2 or fix.shape[1] != self.n:
            raise ValueError("rows_fix must be [nq, n]")
        nq = fix.shape[0]
        rows = (SweepRow * max(1, nq))()
        sw = SweepStats()
        row_ptr = np.zeros(nq + 1, dtype=np.int64)
        thr = 1.0 / self.n if threshold is None else float(threshold)
        self._chk(self._test_entry("fora_hip_test_sweep_rows")(self._ctx, _p(fix), nq, thr, int(max_size), _p(row_ptr), rows, C.byref(sw)))
        out = {"row_ptr": row_ptr, "rows": np.frombuffer(rows, dtype=_SWEEP_ROW_DTYPE, count=nq).copy(), "sweep": sw.as_dict()}
        if want_profile:
            out["ids"], out["cut"], out["vol"] = self.sweep_fetch(int(row_ptr[-1]))
        return out

    def test_sparse_rows(self, rows_fix, threshold=0.0):
        """query_sparse's compaction over caller-made rows ([nq, n] fixed-point words) instead of a query's
        (fora_hip_test_sparse_rows): leaves a held sparse result of chosen row lengths.  Returns (row_ptr, sparse stats)."""
        fix = np.ascontiguousarray(rows_fix, dtype=np.uint64)
        if fix.ndim != 2 or fix.shape[1] != self.n:
            raise ValueError("rows_fix must be [nq, n]")
        nq = fix.shape[0]
        sp = SparseStats()
        row_ptr = np.zeros(nq + 1, dtype=np.int64)
        self._chk(self._test_entry("fora_hip_test_sparse_rows")(self._ctx, _p(fix), nq, float(threshold), _p(row_ptr), C.byref(sp)))
        return row_ptr, sp.as_dict()

    def test_sparse_topk_rows(self, rows_fix, k, threshold=0.0):
        """test_sparse_rows with the top-k selection behind the compaction (fora_hip_test_sparse_topk_rows): leaves the held
        top-k result of the caller's rows.  Returns (row_ptr, sparse stats, topk stats)."""
        fix = np.ascontiguousarray(rows_fix, dtype=np.uint64)
        if fix.ndim != 2 or fix.shape[1] != self.n:
            raise ValueError("rows_fix must be [nq, n]")
        nq = fix.shape[0]
        sp, tk = SparseStats(), TopkStats()
        row_ptr = np.zeros(nq + 1, dtype=np.int64)
        self._chk(self._test_entry("fora_hip_test_sparse_topk_rows")(self._ctx, _p(fix), nq, float(threshold), int(k), _p(row_ptr),
                                                                     C.byref(sp), C.byref(tk)))
        return row_ptr, sp.as_dict(), tk.as_dict()

    def test_sweep_scan(self, diff, vol, nnz):
        """k_sweep_scan on one row (fora_hip_test_sweep_scan): diff (int64 differences of the cuts) and vol (uint64 per
        position) of one length.  Returns (cut uint64 [L], vol uint64 [L], a dict: len, best, cut, vol, den, edges)."""
        cut = np.array(diff, dtype=np.int64)
        v = np.array(vol, dtype=np.uint64)
        if cut.ndim != 1 or cut.shape != v.shape:
            raise ValueError("diff and vol must be one-dimensional and of one length")
        out = np.zeros(6, dtype=np.uint64)
        self._chk(self._test_entry("fora_hip_test_sweep_scan")(self._ctx, _p(cut), _p(v), cut.size, int(nnz), _p(out)))
        return cut.view(np.uint64), v, dict(zip(("len", "best", "cut", "vol", "den", "edges"), (int(x) for x in out)))

    def test_exp(self, t):
        """exp_def of the ROW SOFTMAX contract on the device (fora_hip_test_exp): t a float64 array of points <= 0 (or -inf).
        Returns a float64 array of the same shape."""
        a = np.ascontiguousarray(t, dtype=np.float64)
        out = np.zeros(a.shape, dtype=np.float64)
        self._chk(self._test_entry("fora_hip_test_exp")(self._ctx, _p(a), a.size, _p(out)))
        return out

    def local_cluster(self, sources, with_idx=False, threshold=None, max_size=0):
        """The cluster of least conductance around every source: one int32 id array per source, in sweep order (empty when
        no prefix has a denominator: a dangling source)."""
        r = self.sweep(sources, with_idx=with_idx, threshold=threshold, max_size=max_size, want_profile=True)
        rp, ids = r["row_ptr"], r["ids"]
        return [ids[int(rp[i]):int(rp[i]) + int(r["rows"][i]["best"])].copy() for i in range(len(r["rows"]))]

    def push(self, sources, want=True):
        """want=False: only the per-query stats come back (the slabs stay in HBM)."""
        src = np.ascontiguousarray(sources, dtype=np.int32)
        nq = src.size
        st = (QueryStats * max(1, nq))()
        rsv = np.zeros((nq, self.n), dtype=np.uint64) if want else None
        res = np.zeros((nq, self.n), dtype=np.uint64) if want else None
        self._chk(self._lib.fora_hip_push_batch(self._ctx, _p(src), nq, _p(rsv), _p(res), st))
        if not want:
            return self._stats(st, nq)
        return rsv, res, self._stats(st, nq)

    def topk(self, sources, k, epsilon=0.5, rmax_scale=1.0, with_idx=False):
        src = np.ascontiguousarray(sources, dtype=np.int32)
        nq = src.size
        ids = np.zeros((nq, k), dtype=np.int32)
        sc = np.zeros((nq, k), dtype=np.float64)
        rounds = np.zeros(max(1, nq), dtype=np.int32)
        self._chk(self._lib.fora_hip_topk_batch(self._ctx, _p(src), nq, k, epsilon, rmax_scale, int(with_idx), _p(ids), _p(sc), _p(rounds)))
        return ids, sc, rounds[:nq]

    def set_balanced(self, on=True, start_scale=0.0, c_pop=0.0, c_edge=0.0, t_walk=0.0, t_idx=0.0):
        """--balanced (query.h:848-884); costs <= 0 select the MI355X defaults, start_scale <= 0 the reference's 8."""
        self._chk(self._lib.fora_hip_set_balanced(self._ctx, int(on), start_scale, c_pop, c_edge, t_walk, t_idx))

    def topk_bound(self, sources, k, epsilon=0.5, rmax_scale=1.0, ppr_decay_alpha=0.77, with_idx=False):
        """get_topk without --opt (top-k with bounds, query.h:909-969)."""
        src = np.ascontiguousarray(sources, dtype=np.int32)
        nq = src.size
        ids = np.zeros((nq, k), dtype=np.int32)
        sc = np.zeros((nq, k), dtype=np.float64)
        rounds = np.zeros(max(1, nq), dtype=np.int32)
        self._chk(self._lib.fora_hip_topk_bound_batch(self._ctx, _p(src), nq, k, epsilon, rmax_scale, ppr_decay_alpha, int(with_idx),
                                                      _p(ids), _p(sc), _p(rounds)))
        return ids, sc, rounds[:nq]

    def power_iteration(self, sources, max_iter=100, k=0, want_ppr=True, want_fix=False):
        """Exact SSPPR (gen_exact_topk's fwd_power_iteration, query.h:1192-1238).  Returns (ppr f64 [nq,n] or
        None, ppr raw u64 or None, ids [nq,k] or None, scores or None)."""
        src = np.ascontiguousarray(sources, dtype=np.int32)
        nq = src.size
        ppr = np.zeros((nq, self.n), dtype=np.float64) if want_ppr else None
        fix = np.zeros((nq, self.n), dtype=np.uint64) if want_fix else None
        ids = np.zeros((nq, k), dtype=np.int32) if k else None
        sc = np.zeros((nq, k), dtype=np.float64) if k else None
        self._chk(self._lib.fora_hip_power_iteration_batch(
            self._ctx, _p(src), nq, max_iter, _p(ppr) if want_ppr else None,
            _p(fix) if want_fix else None, k, _p(ids) if k else None, _p(sc) if k else None))
        return ppr, fix, ids, sc

    # ---- baselines (--algo montecarlo / fwdpush)
    def montecarlo(self, sources, epsilon=0.5, k=0, want_ppr=False, want_fix=True):
        """Monte-Carlo SSPPR (montecarlo_query, query.h:16-43): (ppr f64 [nq,n] or None, ppr raw u64 or None,
        ids [nq,k] or None, scores or None, stats)."""
        src = np.ascontiguousarray(sources, dtype=np.int32)
        nq = src.size
        st = (QueryStats * max(1, nq))()
        ppr = np.zeros((nq, self.n), dtype=np.float64) if want_ppr else None
        fix = np.zeros((nq, self.n), dtype=np.uint64) if want_fix else None
        ids = np.zeros((nq, k), dtype=np.int32) if k else None
        sc = np.zeros((nq, k), dtype=np.float64) if k else None
        self._chk(self._lib.fora_hip_montecarlo_batch(self._ctx, _p(src), nq, epsilon, _p(ppr), _p(fix), k, _p(ids), _p(sc), st))
        return ppr, fix, ids, sc, self._stats(st, nq)

    def fwdpush(self, sources, epsilon=0.5, rmax_scale=1.0, k=0, want_ppr=False, want_fix=True):
        """FwdPush (forward_local_update_linear at fwdpush_setting's rmax, ppr = reserve): (ppr f64 or None, reserve raw
        or None, residue raw or None, ids or None, scores or None, stats)."""
        src = np.ascontiguousarray(sources, dtype=np.int32)
        nq = src.size
        st = (QueryStats * max(1, nq))()
        ppr = np.zeros((nq, self.n), dtype=np.float64) if want_ppr else None
        rsv = np.zeros((nq, self.n), dtype=np.uint64) if want_fix else None
        res = np.zeros((nq, self.n), dtype=np.uint64) if want_fix else None
        ids = np.zeros((nq, k), dtype=np.int32) if k else None
        sc = np.zeros((nq, k), dtype=np.float64) if k else None
        self._chk(self._lib.fora_hip_fwdpush_batch(self._ctx, _p(src), nq, epsilon, rmax_scale,
                                                   _p(ppr), _p(rsv), _p(res), k, _p(ids), _p(sc), st))
        return ppr, rsv, res, ids, sc, self._stats(st, nq)

    def bippr(self, sources, epsilon=0.5, rmax_scale=1.0, k=0, want_ppr=False, want_fix=True):
        """BiPPR (bippr_query / bippr_query_topk, query.h:71-193): (ppr f64 [nq,n] or None, ppr raw u64 at 2^60 or None,
        ids [nq,k] or None, scores or None, stats, backward-push counters as a dict)."""
        src = np.ascontiguousarray(sources, dtype=np.int32)
        nq = src.size
        st = (QueryStats * max(1, nq))()
        bwd = BwdStats()
        ppr = np.zeros((nq, self.n), dtype=np.float64) if want_ppr else None
        fix = np.zeros((nq, self.n), dtype=np.uint64) if want_fix else None
        ids = np.zeros((nq, k), dtype=np.int32) if k else None
        sc = np.zeros((nq, k), dtype=np.float64) if k else None
        self._chk(self._lib.fora_hip_bippr_batch(self._ctx, _p(src), nq, epsilon, rmax_scale,
                                                 _p(ppr), _p(fix), k, _p(ids), _p(sc), st, C.byref(bwd)))
        return ppr, fix, ids, sc, self._stats(st, nq), bwd.as_dict()

    def bippr_targets(self, sources, targets, epsilon=0.5, rmax_scale=1.0, want_est=False, want_fix=True):
        """BiPPR for chosen (source, target) sets (fora_hip_bippr_targets_batch): pi(s, t) for every source and every listed
        target, nt backward pushes instead of n.  Returns (est f64 [nq,nt] or None, raw u64 at 2^60 [nq,nt] or None, stats,
        backward-push counters as a dict); fix[i, j] is the word bippr() gives at [i, targets[j]]."""
        src = np.ascontiguousarray(sources, dtype=np.int32)
        tg = np.ascontiguousarray(targets, dtype=np.int32)
        nq, nt = src.size, tg.size
        st = (QueryStats * max(1, nq))()
        bwd = BwdStats()
        est = np.zeros((nq, nt), dtype=np.float64) if want_est else None
        fix = np.zeros((nq, nt), dtype=np.uint64) if want_fix else None
        self._chk(self._lib.fora_hip_bippr_targets_batch(self._ctx, _p(src), nq, _p(tg), nt, epsilon,
                                                         rmax_scale, _p(est), _p(fix), st, C.byref(bwd)))
        return est, fix, self._stats(st, nq), bwd.as_dict()

    @staticmethod
    def _seed_sets(sets, weights):
        """(set_ptr int64, seeds int32, weights float64 or None) of the sets / weights arguments of query_seeds."""
        flat = isinstance(sets, tuple) and len(sets) == 2
        if flat:
            set_ptr = np.ascontiguousarray(sets[0], dtype=np.int64)
            seeds = np.ascontiguousarray(sets[1], dtype=np.int32)
        else:
            sets = [np.asarray(x, dtype=np.int32).reshape(-1) for x in sets]
            set_ptr = np.zeros(len(sets) + 1, dtype=np.int64)
            np.cumsum(np.array([x.size for x in sets], dtype=np.int64), out=set_ptr[1:])
            seeds = np.concatenate(sets).astype(np.int32) if sets else np.zeros(0, dtype=np.int32)
        w = None
        if weights is not None:
            w = weights if flat else (np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in weights])
                                      if len(weights) else np.zeros(0))
            w = np.ascontiguousarray(w, dtype=np.float64)
            if w.size != seeds.size:
                raise ValueError("weights must have the shape of the seeds")
        return set_ptr, seeds, w

    def query_seeds(self, sets, weights=None, with_idx=False, k=0, want_ppr=False, want_fix=True):
        """PPR restarting on weighted seed sets (fora_hip_query_seeds_batch): one row per set, the rows of the seeds combined
        on the GPU.  sets: a LIST of int sequences, one per set, or a 2-TUPLE (set_ptr, seeds) in CSR form -- a tuple of two
        is always read as that pair, so two sets go in a list; weights: the same shape (a list of float sequences, or one
        flat array beside `seeds`), None: uniform.  Returns a dict: fix (raw u64 at 2^62 [ns,n] or None), ppr
        (f64 [ns,n] or None), ids / scores ([ns,k] or None), row_sum_fix (u64 [ns]), stats (a dict)."""
        set_ptr, seeds, w = self._seed_sets(sets, weights)
        ns = set_ptr.size - 1
        st = SeedsStats()
        ppr = np.zeros((ns, self.n), dtype=np.float64) if want_ppr else None
        fix = np.zeros((ns, self.n), dtype=np.uint64) if want_fix else None
        ids = np.zeros((ns, k), dtype=np.int32) if k > 0 else None
        sc = np.zeros((ns, k), dtype=np.float64) if k > 0 else None
        sums = np.zeros(ns, dtype=np.uint64)
        self._chk(self._lib.fora_hip_query_seeds_batch(self._ctx, _p(set_ptr), _p(seeds), _p(w), ns, int(with_idx),
                                                       _p(ppr), _p(fix), k, _p(ids), _p(sc), _p(sums), C.byref(st)))
        return {"fix": fix, "ppr": ppr, "ids": ids, "scores": sc, "row_sum_fix": sums, "stats": st.as_dict()}

    def query_seeds_sparse(self, sets, weights=None, with_idx=False, threshold=None, want_fix=False, device=False):
        """query_seeds() with the rows kept sparse (fora_hip_seeds_sparse_batch + fora_hip_sparse_fetch): node v of set row g
        is kept iff the row's word -- the sum over the set's seeds -- is >= max(1, ceil(threshold * 2^62)); threshold=None:
        1 / n.  sets / weights as for query_seeds.  Returns a dict: row_ptr, ids, vals (a CSR over the sets, ids ascending
        inside a row), fix (the raw words, with want_fix, else None), row_sum_fix (u64 [ns], sums over the WHOLE rows), stats
        (the seeds stats) and sparse (a dict).  device as for query_sparse: torch tensors written on the context's GPU,
        usable with to_torch_csr."""
        set_ptr, seeds, w = self._seed_sets(sets, weights)
        ns = set_ptr.size - 1
        st = SeedsStats()
        sp = SparseStats()
        row_ptr = np.zeros(ns + 1, dtype=np.int64)
        sums = np.zeros(ns, dtype=np.uint64)
        thr = 1.0 / self.n if threshold is None else float(threshold)
        self._chk(self._lib.fora_hip_seeds_sparse_batch(self._ctx, _p(set_ptr), _p(seeds), _p(w), ns, int(with_idx),
                                                        thr, _p(row_ptr), _p(sums), C.byref(st), C.byref(sp)))
        row_ptr, ids, vals, fix = self._sparse_result(row_ptr, int(row_ptr[-1]), want_fix, device, "query_seeds_sparse")
        return {"row_ptr": row_ptr, "ids": ids, "vals": vals, "fix": fix, "row_sum_fix": sums, "stats": st.as_dict(),
                "sparse": sp.as_dict()}

    def query_seeds_sparse_topk(self, sets, k, weights=None, with_idx=False, threshold=None, want_fix=False, device=False):
        """query_seeds_sparse() with every set row cut to its k largest entries on the GPU (fora_hip_seeds_sparse_topk_batch;
        the selection of query_sparse_topk, applied after the sum).  The same dict plus "topk" (the top-k stats)."""
        set_ptr, seeds, w = self._seed_sets(sets, weights)
        ns = set_ptr.size - 1
        st = SeedsStats()
        sp, tk = SparseStats(), TopkStats()
        row_ptr = np.zeros(ns + 1, dtype=np.int64)
        sums = np.zeros(ns, dtype=np.uint64)
        thr = 1.0 / self.n if threshold is None else float(threshold)
        self._chk(self._lib.fora_hip_seeds_sparse_topk_batch(self._ctx, _p(set_ptr), _p(seeds), _p(w), ns, int(with_idx),
                                                             thr, int(k), _p(row_ptr), _p(sums), C.byref(st), C.byref(sp), C.byref(tk)))
        row_ptr, ids, vals, fix = self._sparse_result(row_ptr, int(row_ptr[-1]), want_fix, device, "query_seeds_sparse_topk")
        return {"row_ptr": row_ptr, "ids": ids, "vals": vals, "fix": fix, "row_sum_fix": sums, "stats": st.as_dict(),
                "sparse": sp.as_dict(), "topk": tk.as_dict()}

    def sweep_seeds(self, sets, weights=None, with_idx=False, threshold=None, max_size=0, want_profile=False, device=False):
        """Seed-set expansion (fora_hip_seeds_sweep_batch): sweep() over the rows of query_seeds instead of single sources'.
        sets / weights as for query_seeds, the rest and the returned dict as for sweep, "stats" being the seeds stats."""
        set_ptr, seeds, w = self._seed_sets(sets, weights)
        ns = set_ptr.size - 1
        st = SeedsStats()
        rows = (SweepRow * max(1, ns))()
        sw = SweepStats()
        row_ptr = np.zeros(ns + 1, dtype=np.int64)
        thr = 1.0 / self.n if threshold is None else float(threshold)
        self._chk(self._lib.fora_hip_seeds_sweep_batch(self._ctx, _p(set_ptr), _p(seeds), _p(w), ns, int(with_idx),
                                                       thr, int(max_size), _p(row_ptr), rows, C.byref(st), C.byref(sw)))
        out = {"row_ptr": row_ptr, "rows": np.frombuffer(rows, dtype=_SWEEP_ROW_DTYPE, count=ns).copy(),
               "stats": st.as_dict(), "sweep": sw.as_dict()}
        if want_profile:
            out["ids"], out["cut"], out["vol"] = self.sweep_fetch(int(row_ptr[-1]), device=device)
        return out

    def local_cluster_seeds(self, sets, weights=None, with_idx=False, threshold=None, max_size=0):
        """The cluster of least conductance around every seed set: one int32 id array per set, in sweep order (empty when no
        prefix has a denominator: a set of dangling seeds only)."""
        r = self.sweep_seeds(sets, weights=weights, with_idx=with_idx, threshold=threshold, max_size=max_size, want_profile=True)
        rp, ids = r["row_ptr"], r["ids"]
        return [ids[int(rp[i]):int(rp[i]) + int(r["rows"][i]["best"])].copy() for i in range(len(r["rows"]))]

    # ---- stage hooks
    def bwdpush(self, targets, rmax):
        """Backward push (reverse_local_update_linear, algo.h:703-751) to each target: (reserve u64 [nt,n] at 2^60,
        residue u64 [nt,n] at 2^60, counters as a dict)."""
        tg = np.ascontiguousarray(targets, dtype=np.int32)
        nt = tg.size
        rsv = np.zeros((nt, self.n), dtype=np.uint64)
        res = np.zeros((nt, self.n), dtype=np.uint64)
        bwd = BwdStats()
        self._chk(self._lib.fora_hip_bwdpush_batch(self._ctx, _p(tg), nt, rmax, _p(rsv), _p(res), C.byref(bwd)))
        return rsv, res, bwd.as_dict()

    def walk_counts(self, residue, rsum):
        residue = np.ascontiguousarray(residue, dtype=np.float64)
        out = np.zeros(self.n, dtype=np.uint64)
        N = C.c_uint64(0)
        self._chk(self._lib.fora_hip_walk_counts(self._ctx, _p(residue), rsum, _p(out), C.byref(N)))
        return N.value, out

    def walks(self, stream, rnd, starts, js, no_zero_hop=False):
        starts = np.ascontiguousarray(starts, dtype=np.int32)
        js = np.ascontiguousarray(js, dtype=np.uint64)
        out = np.zeros(starts.size, dtype=np.int32)
        self._chk(self._lib.fora_hip_walks(self._ctx, stream, rnd, int(no_zero_hop), _p(starts), _p(js), starts.size, _p(out)))
        return out

    # ---- measurement
    def set_option(self, name, value):
        self._chk(self._lib.fora_hip_set_option(self._ctx, name.encode(), int(value)))

    def get_option(self, name):
        v = C.c_int64(0)
        self._chk(self._lib.fora_hip_get_option(self._ctx, name.encode(), C.byref(v)))
        return int(v.value)

    def reset_options(self):
        self._chk(self._lib.fora_hip_set_option(self._ctx, b"reset", 0))

    def reset_timing(self):
        self._chk(self._lib.fora_hip_reset_timing(self._ctx))

    def timing(self):
        t = Timing()
        self._chk(self._lib.fora_hip_get_timing(self._ctx, C.byref(t)))
        return t.as_dict()

    def stamps(self):
        """Diagnostic builds (-DFORA_STAMPS): cycles per kernel phase; zeros otherwise."""
        out = np.zeros(32, dtype=np.uint64)
        self._chk(self._lib.fora_hip_get_stamps(self._ctx, _p(out)))
        return out
