"""fora_amd.torch_ops.ppr_attention_fused(backward="fused"): the backward pass of attention over the held rows as one library
call, on the GPU."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_fused_attention_backward_in_one_call():
    """in a fresh child process (tests/torch_ops_attention_bwd_child.py): torch and the library must live on one HIP runtime, so
    the child imports torch before the library is loaded.  The gradients equal Engine.sparse_attention_bwd on the saved float32
    y and the twin, bit for bit, on both paths; only the gradients autograd asks for are made; two heads equal two single-head
    calls side by side; bfloat16 operands get bfloat16 gradients; the gradients agree with float64 autograd of the plain
    expression within the bounds derived for the head-by-head path; a backward pass after the held rows were replaced raises.
    backward="calls" is untouched: tests/test_torch_ops_attention_gpu.py keeps proving that."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "torch_ops_attention_bwd_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    print(r.stdout[-1500:])
    assert "torch ops attention bwd ok" in r.stdout
