"""The numpy twin of COLUMNS (fora_hip_sparse_compact, include/fora_hip.h): the held ids re-expressed over their own columns.
cols is the ascending array of the distinct ids, local[e] the rank of ids[e] in it -- np.unique, nothing else."""
import numpy as np


def compact(ids):
    """(cols, local), both int32: cols = the distinct ids ascending, local[e] = the place of ids[e] in cols"""
    ids = np.asarray(ids, dtype=np.int32).reshape(-1)
    cols, local = np.unique(ids, return_inverse=True)
    return cols.astype(np.int32), np.asarray(local).reshape(-1).astype(np.int32)
