"""The numpy twins of EDGE ATTENTION, BACKWARD and EDGE GAT, BACKWARD (tests/subgraph_attention_bwd_ref.py,
tests/subgraph_gat_ref.py) against a reference that shares nothing with them: torch autograd in float64 on the CPU, built from the
edge list of the crafted subgraph -- a per-group softmax by scatter and index_add, no dense mask (which would merge the duplicate
edge).  The GPU tests hold the kernels to the twins bit for bit; this holds the twins to the mathematics, by row and by column,
within a bound counted rounding by rounding."""
import numpy as np
import pytest

import subgraph_attention_bwd_ref as bw
import subgraph_attention_ref as at
import subgraph_gat_ref as gat
import subgraph_prop_ref as sr
import subgraph_ref

U = 2.0 ** -53
HEADS, D, DV = 2, 5, 3


@pytest.fixture(scope="module")
def graph():
    row_ptr, col, nodes = sr.crafted_graph()
    sub_ptr, sub_col = subgraph_ref.induced(row_ptr, col, nodes)[:2]
    rows, cols = at.groups(sub_ptr, sub_col, "row"), np.asarray(sub_col, dtype=np.int64)
    assert (np.bincount(rows, minlength=sr.CRAFTED_NC) == 0).any() and (np.bincount(cols, minlength=sr.CRAFTED_NC) == 0).any()
    return sub_ptr, sub_col, rows, cols


def _attend(torch, s, group, other, v):
    """out [nc, dv] of one head: the softmax of s inside the groups, times the rows of v at the other end"""
    nc = v.shape[0]
    m = torch.full((nc,), float("-inf"), dtype=torch.float64).scatter_reduce(0, group, s.detach(), "amax")
    e = torch.exp(s - m[group])
    y = e / torch.zeros(nc, dtype=torch.float64).index_add(0, group, e)[group]
    return torch.zeros_like(v).index_add(0, group, y[:, None] * v[other])


def _sum_at(index, values, nc):
    out = np.zeros((nc,) + values.shape[1:])
    np.add.at(out, index, values)
    return out


def _edge_bounds(x, eta_x, y, ge, ve, group, scale):
    """per edge of one head: rho (the relative error of y on either side), ds and its absolute error b, as the docstrings count them.
    x: the scaled score, eta_x: the error of it on either side, ge / ve: the rows of g at the group and of v at the other end"""
    nc = sr.CRAFTED_NC
    L = np.bincount(group, minlength=nc)[group].astype(np.float64)
    segs = np.ceil(L / 256)
    m = np.full(nc, -np.inf)
    np.maximum.at(m, group, x)
    eta = np.zeros(nc)
    np.maximum.at(eta, group, eta_x + 3 * U * np.abs(x) + 2 * U * np.abs(x - m[group]))
    rho = (segs + 16 + L + 4) * U + 2 * eta[group]
    dy = (ge * ve).sum(axis=1)
    a = (ve.shape[1] + 6) * U * np.abs(ge * ve).sum(axis=1)
    T, Dg = _sum_at(group, y * np.abs(dy), nc)[group], _sum_at(group, y * dy, nc)[group]
    eps_D = (L + segs + 12) * U * T + rho * T + _sum_at(group, y * a, nc)[group]
    ds = (dy - Dg) * y * scale
    return rho, ds, (5 * U + rho) * np.abs(ds) + abs(scale) * y * (a + eps_D), L + segs + 2


def _hold(name, got, ref, bound, empty, worst):
    bound = 2 * 1.01 * bound
    err, nz = np.abs(got - ref), bound > 0
    assert (err[~nz] == 0).all(), name                               # no edge, no term: both sides are exactly zero
    for side in (got, ref):                                          # a node without an edge on the summing side: +0.0
        assert not np.ascontiguousarray(side[empty]).view(np.uint64).any(), name
    worst[name] = max(worst.get(name, 0.0), float((err[nz] / bound[nz]).max()))
    assert (err <= bound).all(), (name, worst[name])


@pytest.mark.parametrize("by", ["row", "col"])
def test_the_attention_backward_twin_is_within_the_bound_of_f64_autograd(graph, by):
    """loss = sum(out * G), out[u] = sum over the group of u of softmax(scale <Q[u], K[other]>) V[other]; heads = 2, (d, dv) = (5, 3),
    the twin fed its own forward y64.  Both sides round; the bound holds for EITHER side against exact arithmetic, so the two differ
    by at most twice it.  u = 2^-53; a sum of m terms in any order errs by at most (m - 1) u sum |terms|.  Per (group, head) of L
    edges in segs = ceil(L / 256) segments, as tests/test_attention_bwd_cpu.py counts for the held rows (the per-head bits of the
    subgraph calls are those calls' bits):
    y       within rho = (segs + 16 + L + 4) u + 2 eta relatively: the forward twin's (segs + 16) u + 2 eta and a plain softmax's
            exp, L - 1 adds and a division; eta = max over the group of |scale| (d + 6) u sum_c |q_c k_c| + 3 u |x_e| + 2 u |t_e|,
            the error of exp's argument (the twin adds ceil(d / 64) + 6 times, a plain sum at most d times; t = x - max).
    dy      exact products, at most ceil(dv / 64) + 6 adds in the twin and dv in a plain sum: a_e = (dv + 6) u sum_c |g_c v_ec|.
    D       t_e = y_e dy_e rounds once, then at most 10 + segs adds per path in the twin, L - 1 in a plain sum:
            eps_D = (L + segs + 12) u T + rho T + sum_e y_e a_e, T = sum_e y_e |dy_e|.
    ds      at most five roundings: b_e = (5 u + rho) |ds_e| + |scale| y_e (a_e + eps_D).
    dq      the along sum, L the group's length: a term rounds once, then L - 1 + segs adds:
            (L + segs + 2) u sum_e |ds_e k_ec| + sum_e b_e |k_ec|.
    dk, dv  the across sums, L the length of the OTHER end's group: (L + segs + 2) u sum |ds_e q_c| + sum b_e |q_c| and
            (L + segs + 2) u sum y_e |g_c| + sum rho y_e |g_c|.
    1 % on top for the second-order terms.  Nothing is tuned on what the twin gives.  Largest error / bound measured (by row; by
    column): scale 0.375: dq 0.015, dk 0.006, dv 0.009; dq 0.016, dk 0.009, dv 0.016.  scale -1.75: dq 0.012, dk 0.009, dv 0.013;
    dq 0.016, dk 0.008, dv 0.010."""
    import torch
    sub_ptr, sub_col, rows, cols = graph
    nc = sr.CRAFTED_NC
    group, other = (rows, cols) if by == "row" else (cols, rows)
    rng = np.random.Generator(np.random.PCG64(10800))
    Q, K, V, G = (rng.standard_normal((nc, HEADS * w)).astype(np.float32) for w in (D, D, DV, DV))
    tg, to = torch.tensor(group), torch.tensor(other)
    no_group, no_other = np.bincount(group, minlength=nc) == 0, np.bincount(other, minlength=nc) == 0
    for scale in (0.375, -1.75):
        y64, nan_pairs = at.attention(sub_ptr, sub_col, Q, K, V, heads=HEADS, scale=scale, by=by)[2::2]
        assert nan_pairs == 0
        got = bw.backward(sub_ptr, sub_col, Q, K, V, G, y64, heads=HEADS, scale=scale, by=by)[::2]
        tq, tk, tv = (torch.tensor(X.astype(np.float64), requires_grad=True) for X in (Q, K, V))
        outs = []
        for h in range(HEADS):
            qs, vs = slice(h * D, (h + 1) * D), slice(h * DV, (h + 1) * DV)
            outs.append(_attend(torch, (tq[:, qs][tg] * tk[:, qs][to]).sum(-1) * scale, tg, to, tv[:, vs]))
        (torch.cat(outs, dim=1) * torch.tensor(G.astype(np.float64))).sum().backward()
        ref = [t.grad.numpy() for t in (tq, tk, tv)]
        worst = {}
        Q64, K64, V64, G64 = (X.astype(np.float64) for X in (Q, K, V, G))
        for h in range(HEADS):
            qs, vs = slice(h * D, (h + 1) * D), slice(h * DV, (h + 1) * DV)
            qe, ke, ve, ge = Q64[group, qs], K64[other, qs], V64[other, vs], G64[group, vs]
            x = (qe * ke).sum(axis=1) * scale
            y = y64[h]
            rho, ds, b, adds = _edge_bounds(x, abs(scale) * (D + 6) * U * np.abs(qe * ke).sum(axis=1), y, ge, ve, group, scale)
            xadds = (lambda Lx: Lx + np.ceil(Lx / 256) + 2)(np.bincount(other, minlength=nc)[other].astype(np.float64))
            bq = _sum_at(group, (adds * U * np.abs(ds) + b)[:, None] * np.abs(ke), nc)
            bk = _sum_at(other, (xadds * U * np.abs(ds) + b)[:, None] * np.abs(qe), nc)
            bv = _sum_at(other, (xadds * U * y + rho * y)[:, None] * np.abs(ge), nc)
            for name, n, cs, bound, empty in (("dq", 0, qs, bq, no_group), ("dk", 1, qs, bk, no_other), ("dv", 2, vs, bv, no_other)):
                _hold(name, got[n][:, cs], ref[n][:, cs], bound, empty, worst)
            # the head's slice of the call for both heads is the call for that head alone, bit for bit
            one = bw.backward(sub_ptr, sub_col, Q[:, qs], K[:, qs], V[:, vs], G[:, vs], y64[h:h + 1], heads=1, scale=scale, by=by)[::2]
            for n, cs in enumerate((qs, qs, vs)):
                assert np.array_equal(np.ascontiguousarray(got[n][:, cs]).view(np.uint64), one[n].view(np.uint64))
        print(f"attention by {by} scale={scale}: worst error / bound = " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("slope", [0.2, -0.5])
@pytest.mark.parametrize("by", ["row", "col"])
def test_the_gat_backward_twin_is_within_the_bound_of_f64_autograd(graph, by, slope):
    """loss = sum(out * G), out[u] = sum over the group of u of softmax(leaky_relu(el[row] + er[col], slope)) V[other]: el is read at
    the edge's row and er at its column under both groupings; heads = 2, dv = 3, the twin fed its own forward y64.  z, the f64 sum of
    two f32, is formed by the same addition on both sides and has the same bits, so the select agrees exactly; no |z| is below
    2^-40 here, which keeps autograd's subgradient at 0 out of the comparison.  The bound is the attention twin's (the test above)
    with scale = 1 and the score's own error in eta -- one rounding of z * slope, u |s_e|, in place of the dot product's -- and
    dz      where z < 0, dz = ds * slope rounds once more: b'_e = |slope| b_e + u |dz_e|; where z >= 0 the select adds nothing,
            b'_e = b_e.
    d el, d er  the sums of dz over a row's and over a column's edges (the products with a ones column are exact): a group of L
            edges gives (L + segs + 2) u sum_e |dz_e| + sum_e b'_e, L the length on the side that sums.
    dv      as the attention twin's.
    Largest error / bound measured (by row; by column): slope 0.2: d el 0.018, d er 0.005, dv 0.022; d el 0.012, d er 0.016,
    dv 0.044.  slope -0.5: d el 0.020, d er 0.007, dv 0.018; d el 0.013, d er 0.015, dv 0.034."""
    import torch
    sub_ptr, sub_col, rows, cols = graph
    nc = sr.CRAFTED_NC
    group, other = (rows, cols) if by == "row" else (cols, rows)
    rng = np.random.Generator(np.random.PCG64(10810))
    el, er, V, G = (rng.standard_normal((nc, w)).astype(np.float32) for w in (HEADS, HEADS, HEADS * DV, HEADS * DV))
    z = gat.pre_activation(sub_ptr, sub_col, el, er)
    assert np.abs(z).min() >= 2.0 ** -40
    tg, to, tr, tc = (torch.tensor(i) for i in (group, other, rows, cols))
    no_row, no_col = np.bincount(rows, minlength=nc) == 0, np.bincount(cols, minlength=nc) == 0
    no_other = no_col if by == "row" else no_row
    y64, nan_pairs = gat.forward(sub_ptr, sub_col, el, er, V, heads=HEADS, slope=slope, by=by)[2::2]
    assert nan_pairs == 0
    got = gat.backward(sub_ptr, sub_col, el, er, V, G, y64, heads=HEADS, slope=slope, by=by)[::2]
    tl, te, tv = (torch.tensor(X.astype(np.float64), requires_grad=True) for X in (el, er, V))
    outs = [_attend(torch, torch.nn.functional.leaky_relu(tl[:, h][tr] + te[:, h][tc], slope), tg, to, tv[:, h * DV:(h + 1) * DV]) for h in range(HEADS)]
    (torch.cat(outs, dim=1) * torch.tensor(G.astype(np.float64))).sum().backward()
    ref = [t.grad.numpy() for t in (tl, te, tv)]
    worst = {}
    V64, G64 = V.astype(np.float64), G.astype(np.float64)
    len_row, len_col = (np.bincount(i, minlength=nc).astype(np.float64) for i in (rows, cols))
    for h in range(HEADS):
        hs, vs = slice(h, h + 1), slice(h * DV, (h + 1) * DV)
        ve, ge, y = V64[other, vs], G64[group, vs], y64[h]
        s = np.where(z[h] >= 0, z[h], z[h] * slope)
        rho, ds, b, _ = _edge_bounds(s, U * np.abs(s), y, ge, ve, group, 1.0)
        dz = np.where(z[h] >= 0, ds, ds * slope)
        bz = np.where(z[h] >= 0, b, abs(slope) * b + U * np.abs(dz))
        adds = lambda L: L + np.ceil(L / 256) + 2
        bl = _sum_at(rows, adds(len_row[rows]) * U * np.abs(dz) + bz, nc)[:, None]
        br = _sum_at(cols, adds(len_col[cols]) * U * np.abs(dz) + bz, nc)[:, None]
        xadds = adds((len_col if by == "row" else len_row)[other])
        bv = _sum_at(other, (xadds * U * y + rho * y)[:, None] * np.abs(ge), nc)
        for name, n, cs, bound, empty in (("d el", 0, hs, bl, no_row), ("d er", 1, hs, br, no_col), ("dv", 2, vs, bv, no_other)):
            _hold(name, got[n][:, cs], ref[n][:, cs], bound, empty, worst)
        one = gat.backward(sub_ptr, sub_col, el[:, hs], er[:, hs], V[:, vs], G[:, vs], y64[h:h + 1], heads=1, slope=slope, by=by)[::2]
        for n, cs in enumerate((hs, hs, vs)):
            assert np.array_equal(np.ascontiguousarray(got[n][:, cs]).view(np.uint64), one[n].view(np.uint64))
    print(f"gat by {by} slope={slope}: worst error / bound = " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
