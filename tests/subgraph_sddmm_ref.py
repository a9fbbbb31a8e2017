"""The numpy twin of EDGE SCORES (fora_hip_subgraph_sddmm; include/fora_hip_edge.h): head by head the SCORES (SDDMM) twin of
tests/sddmm_ref.py over the CSR of the held subgraph, on the head's column slice; the narrow element types are widened through
tests/narrow_ref.py (subgraph_prop_ref.widen32)."""
import numpy as np

import sddmm_ref
import subgraph_prop_ref as sr


def scores(sub_ptr, sub_col, A, B, heads=1, a_kind=None, b_kind=None):
    """(out64, out32) [heads, edges]: score[h, e] = <A[row of e], B[sub_col[e]]> over the columns [h * d, (h + 1) * d)"""
    A, B = sr.widen32(A, a_kind), sr.widen32(B, b_kind)
    d = A.shape[1] // heads
    per_head = [sddmm_ref.sddmm_ref(sub_ptr, sub_col, A[:, h * d:(h + 1) * d], B[:, h * d:(h + 1) * d]) for h in range(heads)]
    return np.stack([p[0] for p in per_head]), np.stack([p[1] for p in per_head])
