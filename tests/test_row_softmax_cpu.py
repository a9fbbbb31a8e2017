"""fora_amd.torch_ops.row_softmax on CPU tensors: against torch.softmax row by row, with empty rows and rows of one entry, and
its gradient by torch.autograd.gradcheck in float64.  No GPU and no library call: the function is plain torch."""
import numpy as np
import pytest
import torch

from fora_amd.torch_ops import row_softmax

LENS = [0, 1, 5, 0, 1, 300, 2, 0]


def _rows(dtype, seed):
    g = torch.Generator().manual_seed(seed)
    row_ptr = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    scores = (torch.randn(int(row_ptr[-1]), generator=g, dtype=torch.float64) * 4.0).to(dtype)
    return row_ptr, scores


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_equals_softmax_row_by_row(dtype):
    row_ptr, scores = _rows(dtype, 8400)
    for rp in (row_ptr, torch.from_numpy(row_ptr)):                 # numpy or a tensor
        got = row_softmax(rp, scores)
        assert got.dtype == dtype and got.shape == scores.shape
        eps = torch.finfo(dtype).eps
        for i, L in enumerate(LENS):
            lo, hi = int(row_ptr[i]), int(row_ptr[i + 1])
            want = torch.softmax(scores[lo:hi], dim=0)
            # each side: one rounding per exp (and the subtraction before it, whose error exp turns into a relative one of at
            # most |x| eps <= 32 eps here), at most L eps in the sum of L positive terms however it is ordered, one division
            assert torch.allclose(got[lo:hi], want, rtol=2 * (L + 40) * eps, atol=0.0), i
            if L == 1:
                assert got[lo].item() == 1.0
            if L:
                assert abs(got[lo:hi].sum().item() - 1.0) <= L * eps    # f32 rounding of the row length
    # large scores: the row's max is subtracted before exp
    big = torch.tensor([1000.0, 1001.0, -2000.0, 5.0], dtype=dtype)
    got = row_softmax(np.array([0, 2, 2, 4]), big)
    assert torch.isfinite(got).all() and torch.allclose(got[:2], torch.softmax(big[:2], 0)) and torch.allclose(got[2:], torch.softmax(big[2:], 0))
    # no row at all, and only empty rows
    assert row_softmax(np.array([0]), torch.zeros(0, dtype=dtype)).numel() == 0
    assert row_softmax(np.array([0, 0, 0]), torch.zeros(0, dtype=dtype)).numel() == 0


def test_zero_scores_give_one_over_the_length():
    row_ptr = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    got = row_softmax(row_ptr, torch.zeros(int(row_ptr[-1]), dtype=torch.float32))
    for i, L in enumerate(LENS):
        if L:
            assert (got[int(row_ptr[i]):int(row_ptr[i + 1])].numpy() == np.float32(1.0) / np.float32(L)).all()


def test_gradient():
    row_ptr, scores = _rows(torch.float64, 8500)
    keep = np.concatenate([[0], np.cumsum([0, 1, 5, 0, 3])]).astype(np.int64)       # small rows: gradcheck is quadratic
    x = scores[:int(keep[-1])].clone().requires_grad_(True)
    w = torch.randn(x.numel(), dtype=torch.float64, generator=torch.Generator().manual_seed(8501))
    assert torch.autograd.gradcheck(lambda s: row_softmax(keep, s) * w, (x,), eps=1e-6, atol=1e-7)
