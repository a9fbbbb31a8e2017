"""fora_amd.torch_ops with attention in one library call: ppr_attention_fused and ppr_attention(softmax="fused"), forward and
backward, on the GPU."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_fused_attention_forward_and_backward():
    """in a fresh child process (tests/torch_ops_attention_child.py): torch and the library must live on one HIP runtime, so the
    child imports torch before the library is loaded.  The forward pass equals Engine.sparse_attention and the twin on bits, on
    both paths; the gradients equal the composition of the existing twins on the saved float32 y, head by head; two heads equal
    two single-head calls side by side; "fused" and "engine" agree within the bound of the two float32 roundings the engine
    path makes; the gradients agree with float64 autograd of the plain expression within a bound derived there; a backward
    pass after the held rows were replaced raises."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "torch_ops_attention_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "torch ops attention ok" in r.stdout
