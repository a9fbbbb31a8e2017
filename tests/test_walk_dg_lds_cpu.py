"""LDS budget of the shipped k_walk_dg (CPU, no GPU needed): the static LDS of its bucket-order (XL) instantiations, from the
code-object notes of the shipped library (tools/isa_audit.py), plus the bytes of the headline graph's tables in dynamic LDS,
from make_walk_dg / walk_dg_lds_bytes of fora_amd/csrc/fora_tables.h through tests/walk_dg_lds_tables.cpp.

The shipped shape is three workgroups of 8 waves per CU with a stage of 384 results per wave: static and dynamic LDS of a
workgroup stay within 53 KB (three of them, rounded to the allocation granule, within the CU's 160 KB), the static part
within the 36 KB that leave room for 28 KB of tables under 64 KB (graphs with larger tables than the bench graph's run the
same code), and a wave within 80 VGPRs (6 waves per SIMD)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fora_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LDS_PER_CU = 160 * 1024
WGS_PER_CU = 3
LDS_BUDGET = 53 * 1024        # static + dynamic, per workgroup
LDS_STATIC_BUDGET = 36 * 1024
LDS_GRANULE = 1280            # bytes
BENCH_TABLE_BYTES = 14232     # ws-sized bench graph: H = 256, 221 classes, 4 550 blocks
XL = ["k_walk_dg<%s,%s,true>" % (a, b) for a in ("false", "true") for b in ("false", "true")]


@pytest.fixture(scope="module")
def rows():
    import isa_audit
    from fora_amd import build as b
    return {r["kernel"]: r for r in isa_audit.audit(b.build_hip())}


@pytest.fixture(scope="module")
def bench_tables(tmp_path_factory):
    d = tmp_path_factory.mktemp("dg_lds")
    exe = str(d / "walk_dg_lds_tables")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "walk_dg_lds_tables.cpp")], check=True)
    n, m, row_ptr, col = synth.preset("webstanford", "none")
    path = str(d / "g.csr")
    with open(path, "wb") as f:
        f.write(np.array([n, m], dtype="<i8").tobytes())
        f.write(np.ascontiguousarray(row_ptr, dtype="<i8").tobytes())
        f.write(np.ascontiguousarray(col, dtype="<i4").tobytes())
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return {k: int(v) for k, v in (w.split("=") for w in r.stdout.split())}


def test_bench_graph_tables(bench_tables):
    t = bench_tables
    print(t)
    assert t["have"] == 1 and t["nbx"] > 0
    assert t["lds_xl"] == BENCH_TABLE_BYTES and t["lds_plain"] < t["lds_xl"]


@pytest.mark.parametrize("kernel", XL)
def test_three_workgroups_per_cu_at_the_bench_graph(rows, bench_tables, kernel):
    r = rows[kernel]
    total = r["lds_static"] + bench_tables["lds_xl"]
    granules = (total + LDS_GRANULE - 1) // LDS_GRANULE * LDS_GRANULE
    print(kernel, "static", r["lds_static"], "tables", bench_tables["lds_xl"], "total", total, "allocated", granules, "vgpr", r["vgpr"])
    assert r["lds_static"] <= LDS_STATIC_BUDGET, r["lds_static"]
    assert total <= LDS_BUDGET and WGS_PER_CU * granules <= LDS_PER_CU, (r["lds_static"], total, granules)
    assert 0 < r["vgpr"] <= 80 and r.get("agpr", 0) == 0, r["vgpr"]
