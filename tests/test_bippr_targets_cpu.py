"""Targeted BiPPR on CPU: the header declares fora_hip_bippr_targets_batch with the signature of its contract, the library
exports it, fora_amd.capi binds it and the Engine has bippr_targets.  The GPU runs are in test_bippr_targets_gpu.py."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fora_hip_bippr_targets_batch"


def _header():
    return open(os.path.join(ROOT, "include", "fora_hip.h")).read()


def test_header_declares_the_entry_point_with_its_signature():
    hdr = _header()
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, "no declaration"
    args = [" ".join(re.sub(r"/\*.*?\*/", "", a, flags=re.S).split()) for a in m.group(1).split(",")]
    assert args == ["fora_ctx *ctx", "const int32_t *sources", "int nq", "const int32_t *targets", "int nt",
                    "double epsilon", "double rmax_scale", "double *est_out", "uint64_t *est_fix_out",
                    "fora_query_stats *stats", "fora_bwd_stats *bwd"]
    # the contract paragraph sits next to BIPPR's
    assert hdr.index(" * BIPPR (") < hdr.index(" * TARGETED BIPPR (") < hdr.index(" * SPARSE RESULTS (")


def test_capi_binds_it_and_the_engine_has_bippr_targets():
    from fora_amd import capi
    assert NAME in capi.SYMBOLS
    assert hasattr(capi.Engine, "bippr_targets")
    sig = inspect.signature(capi.Engine.bippr_targets)
    assert list(sig.parameters) == ["self", "sources", "targets", "epsilon", "rmax_scale", "want_est", "want_fix"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["epsilon"], d["rmax_scale"], d["want_est"], d["want_fix"]) == (0.5, 1.0, False, True)


def test_library_exports_it_and_a_null_ctx_is_an_argument_error():
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    fn = getattr(capi.load(), NAME)
    assert fn(None, None, 0, None, 0, 0.5, 1.0, None, None, None, None) == -1  # FORA_E_ARG, answered without a GPU
