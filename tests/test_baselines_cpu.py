"""--algo montecarlo / fwdpush (the reference's baselines, fora.cpp:163) on CPU: the command line takes both names for
query / topk / batch-topk and the C ABI declares both entry points; the runs themselves are in test_baselines_gpu.py."""
import math
import os
import subprocess

import pytest

from test_cli import _write_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORA = os.path.join(ROOT, "fora_amd", "bin", "fora")


@pytest.fixture(scope="module")
def cli():
    import __graft_entry__
    __graft_entry__.build()
    assert os.path.exists(FORA)
    return FORA


def _gpu():
    from fora_amd import capi
    return capi.load().fora_hip_device_count() > 0


@pytest.mark.parametrize("action", ["query", "topk", "batch-topk"])
@pytest.mark.parametrize("algo", ["montecarlo", "fwdpush"])
def test_cli_accepts_baseline_algos(cli, tiny, tmp_path, algo, action):
    folder = tmp_path / "data" / "toy"
    _write_dataset(str(folder), tiny, [1, 2, 3])
    r = subprocess.run([cli, action, "--algo", algo, "--prefix", str(tmp_path / "data") + "/", "--dataset", "toy",
                        "--epsilon", "0.5", "--k", "10", "--result_dir", str(tmp_path / "res")],
                       capture_output=True, text=True, timeout=600)
    assert "Wrong algo param" not in r.stdout and "only --algo fora" not in r.stderr
    assert "config.delta=" in r.stdout and "config.pfail=" in r.stdout   # display_setting, algo.h:341-346
    if not _gpu():  # the run gets as far as the context
        assert r.returncode != 0 and "no usable MI355X" in r.stderr
    else:
        assert r.returncode == 0, r.stderr


def test_cli_help_lists_baselines_and_still_refuses_others(cli):
    r = subprocess.run([cli, "--help"], capture_output=True, text=True)
    algos = r.stdout.split("algo: \n")[1].split("options:")[0].split()
    assert algos == ["fora", "montecarlo", "fwdpush"]
    for action, algo in (("query", "bippr"), ("topk", "hubppr"), ("batch-topk", "mc"), ("query", "")):
        r = subprocess.run([cli, action, "--algo", algo, "--epsilon", "0.5"], capture_output=True, text=True)
        assert r.returncode == 1 and "Wrong algo param" in r.stdout


def test_settings_restated(cli, tiny, tmp_path):
    """montecarlo_setting / fwdpush_setting (algo.h:477-496) in the reference's operand order: the printed values equal
    the Python restatement to the last digit (17 significant digits)."""
    folder = tmp_path / "data" / "toy"
    _write_dataset(str(folder), tiny, [1])
    n, m, eps = tiny.n, tiny.m, 0.3
    delta = pfail = 1.0 / n
    want = {"montecarlo": ("config.omega", 3 * math.log(2 / pfail) / eps / eps / delta),
            "fwdpush": ("config.rmax", 0.5 * delta * eps * n / m)}
    for algo, (key, val) in want.items():
        r = subprocess.run([cli, "query", "--algo", algo, "--prefix", str(tmp_path / "data") + "/", "--dataset", "toy",
                            "--epsilon", str(eps), "--rmax_scale", "0.5", "--result_dir", str(tmp_path / "res")],
                           capture_output=True, text=True, timeout=600)
        line = next(l for l in r.stdout.splitlines() if l.startswith(key + "="))
        assert float(line.split("=")[1]) == val, (algo, line, val)


def test_capi_declares_baselines():
    from fora_amd import capi
    hdr = open(os.path.join(ROOT, "include", "fora_hip.h")).read()
    for name in ("fora_hip_montecarlo_batch", "fora_hip_fwdpush_batch"):
        assert name in capi.SYMBOLS and f"int {name}(" in hdr
    assert hasattr(capi.Engine, "montecarlo") and hasattr(capi.Engine, "fwdpush")
