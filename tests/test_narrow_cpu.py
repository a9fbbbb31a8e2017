"""NARROW OPERANDS on the CPU (the contract of include/fora_hip.h): the numpy twin (tests/narrow_ref.py) against numpy's float16
and torch's FP8 dtypes on every code; the decoders of fora_amd/csrc/fora_narrow.h and the one-byte width table of
fora_amd/csrc/fora_prop_plan.h in a stand-alone program (tests/narrow_plan_check.cpp) under the address and undefined-behaviour
sanitizers -- the sanitized code is that program and nothing else; the header's enumerators and the binding's constants."""
import os
import re
import subprocess

import numpy as np
import pytest

import narrow_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got, want):
    """equal bits, NaN codes compared in NaN-ness"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all()
    assert (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all()


def test_f16_twin_on_every_code():
    codes = np.arange(65536, dtype=np.uint16)
    _same(nr.f16_to_f32(codes), codes.view(np.float16).astype(np.float32))
    assert np.isnan(nr.f16_to_f32(codes)).sum() == 2 * 1023 and np.isinf(nr.f16_to_f32(codes)).sum() == 2


@pytest.mark.parametrize("kind", [nr.E4M3, nr.E5M2])
def test_fp8_twins_on_every_code(kind):
    import torch
    dtype = {nr.E4M3: torch.float8_e4m3fn, nr.E5M2: torch.float8_e5m2}[kind]
    want = torch.arange(256, dtype=torch.uint8).view(dtype).to(torch.float32).numpy()
    got = nr.widen(kind, np.arange(256, dtype=np.uint8))
    _same(got, want)
    if kind == nr.E4M3:
        assert np.isnan(got).sum() == 2 and not np.isinf(got).any() and np.nanmax(got) == 448.0
    else:
        assert np.isnan(got).sum() == 6 and np.isinf(got).sum() == 2
    assert got.view(np.uint32)[0x80] == 0x80000000     # -0 stays -0


def test_moderate_codes_are_finite_and_in_range():
    rng = np.random.Generator(np.random.PCG64(9700))
    for kind in (nr.F16, nr.E4M3, nr.E5M2):
        x = nr.widen(kind, nr.moderate_codes(rng, kind, (50, 7)))
        assert np.isfinite(x).all() and np.abs(x).max() < 8 and (x == 0).any() and (x < 0).any() and (x > 0).any()
        nz = np.abs(x[x != 0])
        assert nz.min() >= 2.0 ** -4


@pytest.fixture(scope="session")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("narrow") / "narrow_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "fora_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "narrow_plan_check.cpp")], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout.strip().splitlines() or [""])[-1] + "\n" + r.stderr[-2000:]
    return r.stdout.split()


def test_the_headers_decoders_on_every_code(plan_check):
    out = _run(plan_check, "decode")
    assert out == ["codes=66048", "ok"], out          # 65536 + 2 * 256


def test_one_byte_widths_against_brute_force(plan_check):
    out = _run(plan_check, "geom")
    assert out == ["cases=51200", "ok"], out          # 32 addresses * 40 pitches * 40 widths
    assert _run(plan_check, "bytes") == ["ok"]


def test_header_and_binding_name_the_three_types():
    import __graft_entry__
    __graft_entry__.build()
    from fora_amd import capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fora_hip.h")).read(), flags=re.S)
    enums = {k: int(v) for body in re.findall(r"\benum\s*\{([^}]*)\}", text) for k, v in re.findall(r"(FORA_PROP_\w+)\s*=\s*(\d+)", body)}
    assert (enums["FORA_PROP_F16"], enums["FORA_PROP_E4M3"], enums["FORA_PROP_E5M2"]) == (4, 5, 6)
    assert (enums["FORA_PROP_F32"], enums["FORA_PROP_BF16"], enums["FORA_PROP_F64"]) == (0, 1, 2)
    assert not [k for k, v in enums.items() if v == 3]                       # 3 stays unassigned
    assert (capi.PROP_F16, capi.PROP_E4M3, capi.PROP_E5M2) == (4, 5, 6)
    assert (capi.PROP_F32, capi.PROP_BF16, capi.PROP_F64) == (0, 1, 2)
    assert nr.PROP_TYPE == {nr.F16: capi.PROP_F16, nr.E4M3: capi.PROP_E4M3, nr.E5M2: capi.PROP_E5M2}
    assert "NARROW OPERANDS" in open(os.path.join(ROOT, "include", "fora_hip.h")).read()
    assert os.path.exists(os.path.join(ROOT, "fora_amd", "csrc", "fora_narrow.h"))
