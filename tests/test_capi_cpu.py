"""CPU checks of the drop-in boundary: the in-tree library loads and exports every
symbol include/fora_hip.h declares; without a GPU the product path refuses to run
(no CPU fallback)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "fora_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fora_hip_\w+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    lib = capi.load()
    names = _declared()
    assert len(names) >= 20
    for s in names:
        assert hasattr(lib, s), s
    assert sorted(capi.SYMBOLS) == names


def test_product_does_not_touch_oracle():
    # the product path must not route through the checker
    for base, _, files in os.walk(os.path.join(ROOT, "fora_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".hpp")):
                text = open(os.path.join(base, f)).read()
                for pat in ("oracle_lib", "-lfora_oracle", '#include "fora_oracle', "include \"../../oracle", "CDLL(os.path.join(ROOT, \"oracle"):
                    assert pat not in text, (f, pat)
                if f != "build.py":  # build.py only compiles the checker, it never loads it
                    assert "libfora_oracle" not in text, f


def test_no_gpu_no_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import fora_amd
    with pytest.raises(fora_amd.ForaError):
        fora_amd.Engine(0)


def test_c_binding_compiles_and_fails_loudly_without_gpu():
    """tests/c_smoke/integration_smoke.c is INTEGRATION.md's reference-side binding as a plain C program (gcc -std=c99,
    -lfora_hip).  Here (no GPU) it must build, link and stop at fora_hip_create with FORA_E_NOGPU -- exit code 77."""
    import subprocess
    from fora_amd import build
    exe = build.build_c_smoke(force=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    import torch
    if not torch.cuda.is_available():
        assert r.returncode == 77, (r.returncode, r.stderr)


def _build_flag(path, name):
    from fora_amd import capi
    v = ctypes.c_int64(-1)
    assert capi.load(path).fora_hip_get_option(None, name.encode(), ctypes.byref(v)) == 0  # a property of the build: no context, no GPU
    return v.value


def test_shipped_library_is_not_a_diagnostic_build():
    """fora_amd/csrc/fora_diag.h: every FORA_PROBE_* / FORA_STAMPS* / FORA_DG_FAKE_* macro turns the library into a
    diagnostic build (some of them compute wrong results on purpose).  The product library must be none of them, and the
    kernel bodies must carry no diagnostic #ifdef of their own -- the hooks live in fora_diag.h."""
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    assert _build_flag(capi.lib_path(), "diag_build") == 0
    assert _build_flag(capi.lib_path(), "test_paths") == 0
    test_lib = os.path.join(ROOT, "fora_amd", "libfora_hip_test.so")
    assert _build_flag(test_lib, "diag_build") == 0 and _build_flag(test_lib, "test_paths") == 1
    for f in ("fora_kernels.h", "fora_exchange.h", "fora_team.h", "fora_hip.hip"):
        text = open(os.path.join(ROOT, "fora_amd", "csrc", f)).read()
        for pat in ("FORA_PROBE_", "FORA_DG_FAKE", "ifdef FORA_STAMPS", "defined(FORA_STAMPS", "FORA_STAGE_PLAIN_STORE",
                    "FORA_DG_PLAIN_ITEMS"):
            assert pat not in text, (f, pat)
    # ... and a context-bound option still needs a context
    v = ctypes.c_int64(0)
    assert capi.load().fora_hip_get_option(None, b"team_fallbacks", ctypes.byref(v)) != 0


# ---- the C ABI, stated once in fora_amd/capi.py (the table _ABI and the struct mirrors), checked once against the header

# sizeof of every struct of include/fora_hip.h, written down so that changing one is a conscious edit
STRUCT_BYTES = {"fora_query_stats": 88, "fora_timing": 184, "fora_bwd_stats": 72, "fora_sparse_stats": 40, "fora_seeds_stats": 48,
                "fora_sweep_row": 48, "fora_sweep_stats": 64, "fora_prop_stats": 56, "fora_propt_stats": 88, "fora_sddmm_stats": 48,
                "fora_softmax_stats": 64, "fora_attn_stats": 72, "fora_attn_grads": 72, "fora_attn_bwd_stats": 120,
                "fora_store_stats": 56, "fora_cols_stats": 32, "fora_topk_stats": 48}


def test_product_rows_of_the_table_are_the_prototypes_of_the_header():
    import abi_header
    from fora_amd import capi
    declared = abi_header.prototypes(abi_header.source(), capi.STRUCTS)
    assert sorted(declared) == _declared() == sorted(capi.SYMBOLS) and len(declared) == 63
    for name, (restype, argtypes) in declared.items():
        test_only, got_restype, got_argtypes = capi.ABI[name]
        assert not test_only, name
        assert got_restype is restype, (name, got_restype, restype)
        assert got_argtypes == argtypes, (name, got_argtypes, argtypes)          # (arity and every type)
    others = {name: capi.ABI[name][1] for name in declared if capi.ABI[name][1] is not ctypes.c_int}
    assert others == {"fora_hip_destroy": None, "fora_hip_last_error": ctypes.c_char_p}


def test_struct_mirrors_have_the_fields_of_the_header():
    import abi_header
    from fora_amd import capi
    declared = abi_header.structs(abi_header.source())
    assert sorted(declared) == sorted(capi.STRUCTS) == sorted(STRUCT_BYTES)
    for name, fields in declared.items():
        assert capi.STRUCTS[name]._fields_ == fields, name                       # (names, order and types; nothing extra either way)
        assert ctypes.sizeof(capi.STRUCTS[name]) == STRUCT_BYTES[name], name
    mirrors = [v for v in vars(capi).values() if isinstance(v, type) and issubclass(v, ctypes.Structure) and hasattr(v, "_fields_")]
    assert sorted(m.__name__ for m in mirrors) == sorted(m.__name__ for m in capi.STRUCTS.values())  # (no mirror outside the check)


def test_struct_mirrors_have_the_c_layout(tmp_path):
    """sizeof and every offsetof of all the structs, from a C compiler"""
    import subprocess
    from fora_amd import capi
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fora_hip.h"', 'int main(void) {']
    for name, mirror in capi.STRUCTS.items():
        lines.append('    printf("%s %%zu", sizeof(%s));' % (name, name))
        lines += ['    printf(" %%zu", offsetof(%s, %s));' % (name, f) for f, _ in mirror._fields_]
        lines.append('    printf("\\n");')
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    got = {row.split()[0]: [int(x) for x in row.split()[1:]] for row in out}
    want = {name: [ctypes.sizeof(m)] + [getattr(m, f).offset for f, _ in m._fields_] for name, m in capi.STRUCTS.items()}
    assert got == want and len(got) == 17


def test_test_only_rows_are_the_definitions_of_the_test_entry_points():
    """the TEST ENTRY POINTS are described in a comment of the header, not declared: their rows are held to their
    definitions; the test library exports each of them, the product library none"""
    import abi_header
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    defined = abi_header.prototypes(abi_header.source(abi_header.HIP_SOURCE), capi.STRUCTS, pattern=r"fora_hip_test_\w+", end="{")
    assert sorted(defined) == sorted(capi.TEST_SYMBOLS) and len(defined) == 5
    assert sorted(capi.ABI) == sorted(capi.SYMBOLS + capi.TEST_SYMBOLS)
    header = open(abi_header.HEADER).read()
    product, test = capi.load(), capi.load(capi.TEST_LIB)
    for name, (restype, argtypes) in defined.items():
        assert capi.ABI[name] == (True, restype, argtypes) and restype is ctypes.c_int, name
        assert name in header and name not in abi_header.source(), name          # (in the comment only)
        assert hasattr(test, name) and not hasattr(product, name), name
    # load() bound the rows: a value of another type is refused at the call, where an unbound function would take anything
    for call in (lambda: test.fora_hip_test_exp(None, None, "0", None), lambda: product.fora_hip_get_option(None, 7, None),
                 lambda: product.fora_hip_sparse_fetch(None, None, None, None, 0.5),
                 lambda: product.fora_hip_get_timing(None, ctypes.byref(capi.SparseStats()))):
        with pytest.raises(ctypes.ArgumentError):
            call()
    assert product.fora_hip_last_error(None) is None or isinstance(product.fora_hip_last_error(None), bytes)
