"""fora_amd.torch_ops with the caller's values on the held pattern: ppr_propagate(values=), ppr_sddmm, ppr_attention and their
backward passes, on the GPU."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_values_operations_and_their_gradients():
    """in a fresh child process (tests/torch_ops_values_child.py): torch and the library must live on one HIP runtime, so the
    child imports torch before the library is loaded.  H.grad, values.grad, A.grad and B.grad equal the twins' results cast
    to f32; a backward pass after sparse_clear raises; ppr_attention with Q = 0 equals the values twin bit for bit."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "torch_ops_values_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "torch ops values ok" in r.stdout
