"""A small parser of the C ABI for the CPU tests: the prototypes and the `typedef struct {...} fora_x;` of
include/fora_hip.h (plain C99, one declaration at a time, no macros inside declarations), each type mapped to ctypes by
the rule fora_amd/capi.py states for its signature table -- so that the table and the struct mirrors are checked
against the header in one place (tests/test_capi_cpu.py).

The rule: int, int32_t, uint32_t, int64_t, uint64_t, double -> the ctypes type of that width; [const] char * ->
c_char_p; fora_ctx * -> c_void_p; fora_ctx ** -> POINTER(c_void_p); a pointer to a fora_* struct -> POINTER(its
mirror); every other pointer -> c_void_p; void (a return type) -> None."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fora_hip.h")
HIP_SOURCE = os.path.join(ROOT, "fora_amd", "csrc", "fora_hip.hip")
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
           "double": C.c_double}


def source(path=HEADER):
    """the file without comments and preprocessor lines"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(path).read(), flags=re.S)
    return re.sub(r"(?m)^\s*#.*$", "", text)


def ctype_of(decl, mirrors):
    """The ctypes type of one declaration without its commas: `const int64_t *row_ptr`, `fora_ctx **`, `int`.  mirrors:
    {C struct name: ctypes.Structure}."""
    stars = decl.count("*")
    base = [w for w in decl.replace("*", " ").split() if w != "const"][0]  # (a second word is the declared name)
    if base == "fora_ctx":
        return {1: C.c_void_p, 2: C.POINTER(C.c_void_p)}[stars]
    if base.startswith("fora_"):
        assert stars == 1, decl
        return C.POINTER(mirrors[base])
    if stars == 0:
        return None if base == "void" else SCALARS[base]
    assert stars == 1, decl
    return C.c_char_p if base == "char" else C.c_void_p


def prototypes(text, mirrors, pattern=r"fora_hip_\w+", end=";"):
    """{name: (restype, [argtypes])} of every `type name(params)<end>` whose name matches pattern; end="{": definitions"""
    out = {}
    for ret, name, params in re.findall(r"(?m)^((?:const\s+)?\w+[\s*]+)(%s)\s*\(([^()]*)\)\s*%s" % (pattern, re.escape(end)), text):
        params = [p for p in params.split(",") if p.strip() not in ("", "void")]
        assert name not in out, name
        out[name] = (ctype_of(ret, mirrors), [ctype_of(p, mirrors) for p in params])
    return out


def structs(text, mirrors=None):
    """{struct name: [(field, ctypes type)]} of every `typedef struct {...} fora_x;`; `uint64_t a, b;` declares two
    fields, a pointer field is c_void_p"""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{([^{}]*)\}\s*(fora_\w+)\s*;", text):
        fields = []
        for decl in (d.strip() for d in body.split(";")):
            if decl:
                base, rest = re.match(r"((?:const\s+)?\w+)(.*)", decl, flags=re.S).groups()
                fields += [(d.strip("* \n\t"), ctype_of(base + " " + "*" * d.count("*"), mirrors or {})) for d in rest.split(",")]
        out[name] = fields
    return out
