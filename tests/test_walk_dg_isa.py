"""Register file of every k_walk_dg instantiation the launch can select (NZH x BITS32 x XL), from the code-object notes of the
shipped library (tools/isa_audit.py; CPU, no GPU needed): no VGPR spills, no scratch, and at most 80 VGPRs -- 6 waves per
SIMD, the occupancy the kernel's 512-thread workgroups and its LDS share are laid out for."""
import itertools
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

INSTANCES = ["k_walk_dg<%s,%s,%s>" % tuple("true" if b else "false" for b in bits)
             for bits in itertools.product((False, True), repeat=3)]


@pytest.fixture(scope="module")
def rows():
    import isa_audit
    from fora_amd import build as b
    lib = b.build_hip()
    return {r["kernel"]: r for r in isa_audit.audit(lib)}


@pytest.mark.parametrize("kernel", INSTANCES)
def test_walk_dg_register_file(rows, kernel):
    assert kernel in rows, sorted(k for k in rows if k.startswith("k_walk_dg"))
    r = rows[kernel]
    assert r["vgpr_spill"] == 0 and r["scratch_bytes"] == 0 and r["scratch"] == 0, r
    assert 0 < r["vgpr"] <= 80, r["vgpr"]
    assert r.get("agpr", 0) == 0
    # static LDS next to at most 28 KB of dynamic tables (build_walk_dg's bound): 64 KB per workgroup
    assert r["lds_static"] + 28 * 1024 <= 64 * 1024, r["lds_static"]


def test_no_other_instantiation_is_built(rows):
    assert sorted(k for k in rows if k.startswith("k_walk_dg")) == sorted(INSTANCES)
