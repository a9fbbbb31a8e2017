"""fora_amd.torch_ops with the softmax in the library: ppr_row_softmax and ppr_attention(softmax="engine"), forward and
backward, on the GPU."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_row_softmax_and_attention_through_the_engine():
    """in a fresh child process (tests/torch_ops_softmax_child.py): torch and the library must live on one HIP runtime, so the
    child imports torch before the library is loaded.  ppr_row_softmax's output and gradient equal the twins' f32 results;
    ppr_attention(softmax="engine") equals the composition of the SDDMM, softmax and values twins in both directions; the
    engine and torch settings agree within the stated f32 bound; a backward pass after sparse_clear raises."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "torch_ops_softmax_child.py")], capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(here))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "torch ops softmax ok" in r.stdout
