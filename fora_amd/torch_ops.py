"""torch.autograd over the held sparse rows: Z = PI * H forward (Engine.sparse_propagate), dL/dH = PI^T * dL/dZ backward
(Engine.sparse_propagate_t), both on the rows the engine holds -- the propagation step of an APPNP / PPRGo style model whose
rows are computed once and whose H = MLP(X) changes at every step.  With the caller's values on the held pattern
(ppr_propagate(values=), ppr_sddmm, ppr_row_softmax, row_softmax, ppr_attention, ppr_attention_fused) the three operations are each other's gradients, so
attention over the held neighbourhoods, a learned temperature or a re-weighting stay inside the library.  Import torch before the first Engine is created, so that
the library and torch share one HIP runtime.  fora_amd/__init__.py does not import this module: the package needs no torch.
Wherever an operand or a gradient below has n rows, n is the engine's held column count (Engine.held_cols): the nodes of the
graph, or, after Engine.sparse_compact / store_take_compact, the nc nodes `cols` that the held rows touch -- pass X[cols] and
autograd carries the gradient back through that index.  A compaction between a forward and its backward pass makes the
backward pass raise, like any other change of the held rows.
subgraph_propagate is message passing over the graph's own edges among those nc nodes (Engine.sparse_subgraph): A_S x X and
A_S^T x X, each the other's gradient.  subgraph_sddmm scores every edge of that subgraph, all heads in one call, and
subgraph_propagate_values is the product with learnable edge weights: the scores and the two products are each other's
gradients, as ppr_sddmm and ppr_propagate(values=) are on the held rows.  subgraph_edge_softmax is the softmax over each
node's out- or in-edges between the two, and subgraph_attention composes the three."""
import torch


class _PprPropagate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, H, engine, row_ptr, normalize):
        out32, _, _ = engine.sparse_propagate(row_ptr, H.detach(), normalize=normalize, want32=True, want64=False)
        ctx.engine, ctx.row_ptr, ctx.normalize, ctx.dtype = engine, row_ptr, normalize, H.dtype
        ctx.generation = engine.get_option("sparse_generation")
        return out32

    @staticmethod
    def backward(ctx, G):
        engine = ctx.engine
        if engine.get_option("sparse_generation") != ctx.generation:
            raise RuntimeError("ppr_propagate: the engine's held sparse result was replaced or cleared after the forward pass; "
                               "the backward pass needs the rows the forward pass used")
        G = _dense_operand(G)  # (an expanded or transposed gradient is copied; a row-strided one is read in place)
        out32, _, _ = engine.sparse_propagate_t(ctx.row_ptr, G, normalize=ctx.normalize, want32=True, want64=False)
        return (out32 if ctx.dtype == torch.float32 else out32.to(ctx.dtype)), None, None, None


def _held_guard(ctx_gen, engine, who):
    if engine.get_option("sparse_generation") != ctx_gen:
        raise RuntimeError(f"{who}: the engine's held sparse result was replaced or cleared after the forward pass; "
                           "the backward pass needs the rows the forward pass used")


_FP8 = (torch.float8_e4m3fn, torch.float8_e5m2)


def _dense_operand(X):
    """a gradient as the library reads it: float32, bfloat16 or float16, [rows, d], column stride one element"""
    if X.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        X = X.to(torch.float32)
    if X.dim() != 2 or (X.shape[1] > 1 and X.stride(1) != 1) or (X.shape[0] > 1 and X.stride(0) < X.shape[1]):
        X = X.contiguous()
    return X


def _refuse_fp8_grad(who, **operands):
    """an FP8 tensor is a constant operand (the library reads it as it lies): one that asks for a gradient is refused before
    anything runs -- the gradient would have to be rounded to 8 bits, which is the caller's decision and scaling"""
    for name, X in operands.items():
        if torch.is_tensor(X) and X.dtype in _FP8 and X.requires_grad:
            raise ValueError(f"{who}: {name} is an FP8 tensor that requires grad; an FP8 operand is a constant -- keep the "
                             "parameter in a wider dtype and pass its FP8 copy detached")


def _entry_values(g):
    """a gradient per entry as the values of a product: float32 or float64, contiguous"""
    if g.dtype not in (torch.float32, torch.float64):
        g = g.to(torch.float32)
    return g.contiguous()


class _PprPropagateValues(torch.autograd.Function):
    """Z = P(values) x H: dH = P(values)^T x G (the _t_vals product), dvalues = sddmm(G, H)"""

    @staticmethod
    def forward(ctx, H, values, engine, row_ptr):
        out32, _, _ = engine.sparse_propagate(row_ptr, H.detach(), want32=True, want64=False, values=values.detach())
        ctx.save_for_backward(H, values)
        ctx.engine, ctx.row_ptr = engine, row_ptr
        ctx.generation = engine.get_option("sparse_generation")
        return out32

    @staticmethod
    def backward(ctx, G):
        H, values = ctx.saved_tensors
        engine = ctx.engine
        _held_guard(ctx.generation, engine, "ppr_propagate")
        G = _dense_operand(G)
        dH = dv = None
        if ctx.needs_input_grad[0]:
            dH, _, _ = engine.sparse_propagate_t(ctx.row_ptr, G, want32=True, want64=False, values=values.detach())
            dH = dH if H.dtype == torch.float32 else dH.to(H.dtype)
        if ctx.needs_input_grad[1]:
            dv, _, _ = engine.sparse_sddmm(ctx.row_ptr, G, H.detach(), want32=True, want64=False)
            dv = dv if values.dtype == torch.float32 else dv.to(values.dtype)
        return dH, dv, None, None


class _PprSddmm(torch.autograd.Function):
    """scores = sddmm(A, B): dA = P(g) x B (the _vals product), dB = P(g)^T x A (the _t_vals product)"""

    @staticmethod
    def forward(ctx, A, B, engine, row_ptr):
        out32, _, _ = engine.sparse_sddmm(row_ptr, A.detach(), B.detach(), want32=True, want64=False)
        ctx.save_for_backward(A, B)
        ctx.engine, ctx.row_ptr = engine, row_ptr
        ctx.generation = engine.get_option("sparse_generation")
        return out32

    @staticmethod
    def backward(ctx, g):
        A, B = ctx.saved_tensors
        engine = ctx.engine
        _held_guard(ctx.generation, engine, "ppr_sddmm")
        g = _entry_values(g)
        dA = dB = None
        if ctx.needs_input_grad[0]:
            dA, _, _ = engine.sparse_propagate(ctx.row_ptr, B.detach(), want32=True, want64=False, values=g)
            dA = dA if A.dtype == torch.float32 else dA.to(A.dtype)
        if ctx.needs_input_grad[1]:
            dB, _, _ = engine.sparse_propagate_t(ctx.row_ptr, A.detach(), want32=True, want64=False, values=g)
            dB = dB if B.dtype == torch.float32 else dB.to(B.dtype)
        return dA, dB, None, None


def ppr_propagate(engine, row_ptr, H, normalize=False, values=None):
    """Z = (held sparse rows of `engine`) x H as a differentiable torch operation.  row_ptr: as query_sparse /
    query_seeds_sparse returned it (a numpy array or a tensor).  H: [n, d] (n = engine.held_cols) float32, bfloat16 or float16 on the
    engine's GPU (or FP8 -- float8_e4m3fn, float8_e5m2 -- as a constant: one that requires grad is a ValueError), column stride one element.  Returns Z [nq, d] float32 on the device; Z.backward(G) leaves H.grad = (held rows)^T x G in H's
    dtype.  The rows must still be held when the backward pass runs: a query_sparse, query_seeds_sparse, store_take,
    sparse_compact, sparse_clear or set_graph in between makes it raise.
    values: a float32 or float64 tensor of `entries` elements on the device, one per held entry in held order, used as the
    weights in place of the PPR values (Engine.sparse_propagate(values=)); the result is then differentiable in both H and
    values -- H.grad by the transposed product with the same values, values.grad = ppr_sddmm(G, H).  Not together with
    normalize.  values=None is the code path this function always had."""
    _refuse_fp8_grad("ppr_propagate", H=H)
    if values is None:
        return _PprPropagate.apply(H, engine, row_ptr, bool(normalize))
    if normalize:
        raise ValueError("ppr_propagate: normalize and values exclude each other (a division is the caller's: see row_softmax)")
    return _PprPropagateValues.apply(H, values, engine, row_ptr)


class _SubgraphPropagate(torch.autograd.Function):
    """Y = A_S x X (transposed: A_S^T x X) over the held subgraph; dX = the opposite product of G, after G's rows were divided
    by the forward counts when the forward call took the mean"""

    @staticmethod
    def forward(ctx, X, engine, values, mean, transposed):
        fwd = engine.subgraph_propagate_t if transposed else engine.subgraph_propagate
        out32, _, _ = fwd(X.detach(), values=values, mean=mean, want32=True, want64=False)
        ctx.engine, ctx.values, ctx.mean, ctx.transposed, ctx.dtype = engine, values, mean, transposed, X.dtype
        ctx.generation = engine.get_option("sparse_generation")
        return out32

    @staticmethod
    def backward(ctx, G):
        engine = ctx.engine
        _held_guard(ctx.generation, engine, "subgraph_propagate")
        G = _dense_operand(G)
        if ctx.mean:
            cnt = engine.subgraph_degrees(transposed=ctx.transposed, device=True).clamp(min=1)
            G = (G.to(torch.float64) / cnt.to(torch.float64)[:, None]).to(torch.float32)
        bwd = engine.subgraph_propagate if ctx.transposed else engine.subgraph_propagate_t
        out32, _, _ = bwd(G, values=ctx.values, want32=True, want64=False)
        return (out32 if ctx.dtype == torch.float32 else out32.to(ctx.dtype)), None, None, None, None


def subgraph_propagate(engine, X, values=None, norm=None, direction="out"):
    """One message-passing step over the subgraph `engine` holds (Engine.sparse_subgraph) as a differentiable torch operation.
    X: [nc, d] (nc = engine.held_cols) float32, bfloat16 or float16 on the engine's GPU (or FP8 as a constant: one that requires
    grad is a ValueError), column stride one element.  direction "out": Y = A_S x X, every node sums its out-neighbours inside
    the batch (Engine.subgraph_propagate); "in": Y = A_S^T x X, its in-neighbours (Engine.subgraph_propagate_t).  Returns Y
    [nc, d] float32 on the device; the backward pass is the opposite call on the gradient G, so X.grad has defined bits too.
    values: one float32 or float64 per edge of the subgraph in the order of sub_col (a tensor on the device or a numpy array),
    used as the weights in both passes; it is a constant here -- a values tensor that requires grad is a ValueError (its
    gradient is an SDDMM over the subgraph's edges: subgraph_propagate_values is the product with learnable weights).
    norm="mean" (not together with values): every output row is divided by the number of its terms.  The backward pass is
    then DEFINED as this composition: count_j = the number of terms of forward row j (at least 1), G'[j] =
    float32(float64(G[j]) / float64(count_j)) in torch, X.grad = the plain (unit-weight, no mean) opposite product of G'.
    The subgraph must still be held when the backward pass runs: a call that replaces or clears the held rows in between
    makes it raise."""
    if direction not in ("out", "in"):
        raise ValueError('subgraph_propagate: direction is "out" or "in"')
    if norm not in (None, "mean"):
        raise ValueError('subgraph_propagate: norm is None or "mean"')
    _refuse_fp8_grad("subgraph_propagate", X=X)
    if torch.is_tensor(values):
        if values.requires_grad:
            raise ValueError("subgraph_propagate: values is a constant here; a values tensor that requires grad is not supported "
                             "(its gradient is an SDDMM over the subgraph's edges: call subgraph_propagate_values)")
        values = _entry_values(values.detach())
    if norm == "mean" and values is not None:
        raise ValueError("subgraph_propagate: norm and values exclude each other (pass the normalisation as values)")
    return _SubgraphPropagate.apply(X, engine, values, norm == "mean", direction == "in")


def _as_leaf_dtype(g, X):
    return g if g is None or X.dtype == torch.float32 else g.to(X.dtype)


class _SubgraphPool(torch.autograd.Function):
    """Y = max / min of X over each node's group of the held subgraph; dX = the one backward call over the arg the forward kept"""

    @staticmethod
    def forward(ctx, X, engine, op, by):
        out32, _, arg, _ = engine.subgraph_pool(X.detach(), op=op, by=by, want32=True, want64=False, want_arg=True)
        ctx.engine, ctx.by, ctx.arg, ctx.leaf = engine, by, arg, X.new_empty(0)   # (arg: int32 [nc, d] on the device; leaf: X's dtype)
        ctx.generation = engine.get_option("sparse_generation")
        return out32

    @staticmethod
    def backward(ctx, G):
        _held_guard(ctx.generation, ctx.engine, "subgraph_pool")
        out32, _, _ = ctx.engine.subgraph_pool_bwd(_dense_operand(G), ctx.arg, by=ctx.by, want32=True, want64=False)
        return _as_leaf_dtype(out32, ctx.leaf), None, None, None


def subgraph_pool(engine, X, op="max", direction="out"):
    """Max or min pooling over the subgraph `engine` holds (Engine.sparse_subgraph) as a differentiable torch operation: Y[j, c] =
    the maximum (op="min": the minimum) of X[v, c] over the out-neighbours v of node j inside the batch (direction "out":
    Engine.subgraph_pool by row) or over its in-neighbours ("in": by column); a node without neighbours gets 0.  X: [nc, d]
    (nc = engine.held_cols) float32, bfloat16 or float16 on the engine's GPU (or FP8 as a constant: one that requires grad is a
    ValueError), column stride one element.  Returns Y [nc, d] float32 on the device.
    The tie rule: the winner of (j, c) is the FIRST edge of the group -- by its place in sub_col -- among those that hold the
    extreme value, -0.0 and +0.0 counting as equal; a NaN beats every number, the first NaN wins.  The backward pass gives the
    WHOLE gradient G[j, c] to that first extremal edge's source node and nothing to the others that tie with it.  This differs
    from torch.scatter_reduce(..., "amax" / "amin"), whose backward pass splits the gradient evenly over the tied entries;
    here X.grad is an ordered float64 sum per element, rounded once, so every bit of it is defined.  The forward pass keeps
    the winners as an int32 tensor on the device, and the backward pass is one call over it.  The subgraph must still be held
    when the backward pass runs: a call that replaces or clears the held rows in between makes it raise."""
    if direction not in ("out", "in"):
        raise ValueError('subgraph_pool: direction is "out" or "in"')
    if op not in ("max", "min"):
        raise ValueError('subgraph_pool: op is "max" or "min"')
    _refuse_fp8_grad("subgraph_pool", X=X)
    return _SubgraphPool.apply(X, engine, op, "row" if direction == "out" else "col")


class _SubgraphSddmm(torch.autograd.Function):
    """scores[h] = sddmm over the subgraph's edges of the head's column slices of A and B; per head, with g_h the gradient of
    its scores as values: dA[:, slice] = A_S(g_h) x B[:, slice], dB[:, slice] = A_S(g_h)^T x A[:, slice], written in place"""

    @staticmethod
    def forward(ctx, A, B, engine, heads):
        out32, _, _ = engine.subgraph_sddmm(A.detach(), B.detach(), heads=heads, want32=True, want64=False)
        ctx.save_for_backward(A, B)
        ctx.engine, ctx.heads = engine, heads
        ctx.generation = engine.get_option("sparse_generation")
        return out32

    @staticmethod
    def backward(ctx, g):
        A, B = ctx.saved_tensors
        engine, heads = ctx.engine, ctx.heads
        _held_guard(ctx.generation, engine, "subgraph_sddmm")
        g = _entry_values(g)
        d = A.shape[1] // heads
        Ad, Bd = A.detach(), B.detach()
        dA = torch.empty(A.shape, dtype=torch.float32, device=A.device) if ctx.needs_input_grad[0] else None
        dB = torch.empty(B.shape, dtype=torch.float32, device=B.device) if ctx.needs_input_grad[1] else None
        for h in range(heads):
            cs = slice(h * d, (h + 1) * d)
            if dA is not None:
                engine.subgraph_propagate(Bd[:, cs], values=g[h], want64=False, out32=dA[:, cs])
            if dB is not None:
                engine.subgraph_propagate_t(Ad[:, cs], values=g[h], want64=False, out32=dB[:, cs])
        return _as_leaf_dtype(dA, A), _as_leaf_dtype(dB, B), None, None


def subgraph_sddmm(engine, A, B, heads=1):
    """scores[h, e] = <A[row of e], B[sub_col[e]]> over the columns [h * d, (h + 1) * d) for every edge e of the subgraph
    `engine` holds (Engine.subgraph_sddmm, the EDGE SCORES contract), float32 [heads, edges] on the device: edge gates, link
    scores, the scores of an attention layer over the sampled graph.  A, B: [nc, heads * d] (nc = engine.held_cols) float32,
    bfloat16 or float16 tensors on the engine's GPU (or FP8 as constants: one that requires grad is a ValueError), column
    stride one element.  Differentiable in A and B: with g_h the gradient of head h's scores, A.grad[:, slice] =
    A_S(g_h) x B[:, slice] and B.grad[:, slice] = A_S(g_h)^T x A[:, slice] -- the two subgraph products with values = g_h on
    the head's column slice, written in place -- in the leaf's dtype.  The subgraph must still be held when the backward pass
    runs."""
    heads = int(heads)
    if heads < 1 or A.dim() != 2 or A.shape[1] % heads:
        raise ValueError("subgraph_sddmm: heads must be at least 1 and divide the columns of A and B")
    _refuse_fp8_grad("subgraph_sddmm", A=A, B=B)
    return _SubgraphSddmm.apply(A, B, engine, heads)


class _SubgraphPropagateValues(torch.autograd.Function):
    """Y = A_S(values) x X (transposed: A_S(values)^T x X); dX = the opposite product of G with the same values; dvalues =
    subgraph_sddmm(G, X) (transposed: subgraph_sddmm(X, G)) -- the operand read at the edge's row comes first"""

    @staticmethod
    def forward(ctx, X, values, engine, transposed):
        fwd = engine.subgraph_propagate_t if transposed else engine.subgraph_propagate
        out32, _, _ = fwd(X.detach(), values=values.detach(), want32=True, want64=False)
        ctx.save_for_backward(X, values)
        ctx.engine, ctx.transposed = engine, transposed
        ctx.generation = engine.get_option("sparse_generation")
        return out32

    @staticmethod
    def backward(ctx, G):
        X, values = ctx.saved_tensors
        engine = ctx.engine
        _held_guard(ctx.generation, engine, "subgraph_propagate_values")
        G = _dense_operand(G)
        dX = dv = None
        if ctx.needs_input_grad[0]:
            bwd = engine.subgraph_propagate if ctx.transposed else engine.subgraph_propagate_t
            dX, _, _ = bwd(G, values=values.detach(), want32=True, want64=False)
        if ctx.needs_input_grad[1]:
            a, b = (X.detach(), G) if ctx.transposed else (G, X.detach())
            dv, _, _ = engine.subgraph_sddmm(a, b, heads=1, want32=True, want64=False)
            dv = dv[0]
        return _as_leaf_dtype(dX, X), dv, None, None


def subgraph_propagate_values(engine, X, values, direction="out"):
    """subgraph_propagate with LEARNABLE edge weights: Y = A_S(values) x X (direction "out") or A_S(values)^T x X ("in") over
    the subgraph `engine` holds, float32 [nc, d] on the device, differentiable in X and in values.  X: as for
    subgraph_propagate.  values: a float32 tensor of one element per edge of the subgraph in the order of sub_col, on the
    engine's GPU.  X.grad is the opposite product of the gradient G with the same values; values.grad[e] =
    <G[row of e], X[sub_col[e]]> for "out" and <X[row of e], G[sub_col[e]]> for "in" (Engine.subgraph_sddmm with the operands
    in that order), float32, every bit defined.  The subgraph must still be held when the backward pass runs."""
    if direction not in ("out", "in"):
        raise ValueError('subgraph_propagate_values: direction is "out" or "in"')
    if not torch.is_tensor(values) or values.dtype != torch.float32 or values.dim() != 1:
        raise ValueError("subgraph_propagate_values: values is a float32 tensor of one element per edge")
    _refuse_fp8_grad("subgraph_propagate_values", X=X)
    return _SubgraphPropagateValues.apply(X, values, engine, direction == "in")


class _SubgraphEdgeSoftmax(torch.autograd.Function):
    """y = the softmax of scores * scale inside every group of the subgraph's edges (Engine.subgraph_softmax), y32 saved;
    dscores = ((g - sum_group(y g)) y) scale (Engine.subgraph_softmax_bwd)"""

    @staticmethod
    def forward(ctx, scores, engine, scale, by):
        s = scores.detach()
        if s.dtype not in (torch.float32, torch.float64):
            s = s.to(torch.float32)
        y32, _, _ = engine.subgraph_softmax(s, scale=scale, by=by, want32=True, want64=False)
        ctx.save_for_backward(y32)
        ctx.engine, ctx.scale, ctx.by, ctx.dtype = engine, scale, by, scores.dtype
        ctx.generation = engine.get_option("sparse_generation")
        return y32

    @staticmethod
    def backward(ctx, g):
        (y32,) = ctx.saved_tensors
        _held_guard(ctx.generation, ctx.engine, "subgraph_edge_softmax")
        dx, _, _ = ctx.engine.subgraph_softmax_bwd(y32, _entry_values(g), scale=ctx.scale, by=ctx.by, want32=True, want64=False)
        return (dx if ctx.dtype == torch.float32 else dx.to(ctx.dtype)), None, None, None


def subgraph_edge_softmax(engine, scores, scale=1.0, by="row"):
    """softmax of scores * scale over each node's edges of the subgraph `engine` holds, head by head (Engine.subgraph_softmax,
    the EDGE SOFTMAX contract: the defined exp and fixed order of ppr_row_softmax, every bit defined), float32 [heads, edges]
    on the device.  scores: [heads, edges] in the order of sub_col -- what subgraph_sddmm returns -- a float32 or float64
    tensor on the engine's GPU; the gradient comes back in its dtype.  by="row": over the out-edges of a node, the groups
    subgraph_propagate_values(direction="out") sums over; by="col": over its in-edges, the groups of direction="in".  The
    backward pass is Engine.subgraph_softmax_bwd on the saved float32 output.  scale is a number, not a differentiable
    operand.  The subgraph must still be held when the backward pass runs."""
    if by not in ("row", "col"):
        raise ValueError('subgraph_edge_softmax: by is "row" or "col"')
    if not torch.is_tensor(scores) or scores.dim() != 2:
        raise ValueError("subgraph_edge_softmax: scores is a [heads, edges] tensor")
    return _SubgraphEdgeSoftmax.apply(scores, engine, float(scale), by)


def subgraph_attention(engine, Q, K, V, heads=1, scale=None, direction="out"):
    """Attention over the sampled graph, every step a call of the library with defined bits: the composition of
    subgraph_sddmm, subgraph_edge_softmax and, per head, subgraph_propagate_values -- no backward code of its own.
    direction="out": node j attends over its out-edges, out[j] = sum over the edges e of row j of y[e] * V[sub_col[e]] with
    y = softmax over the row of scale * <Q[j], K[sub_col[e]]>.  direction="in": node v attends over its in-edges, out[v] =
    sum over the edges e with sub_col[e] == v of y[e] * V[row of e] with y = softmax over the column of scale *
    <Q[v], K[row of e]> (the scores are subgraph_sddmm(K, Q): a is read at the edge's row).  Q, K: [nc, heads * d], V:
    [nc, heads * dv], float32, bfloat16 or float16 tensors on the engine's GPU (FP8 as constants); scale: d ** -0.5 when
    None.  Returns float32 [nc, heads * dv], differentiable in Q, K and V.  subgraph_attention_fused is the same layer with
    the forward pass in one library call."""
    heads = int(heads)
    if direction not in ("out", "in"):
        raise ValueError('subgraph_attention: direction is "out" or "in"')
    if heads < 1 or Q.dim() != 2 or V.dim() != 2 or Q.shape[1] % heads or V.shape[1] % heads:
        raise ValueError("subgraph_attention: heads must be at least 1 and divide the columns of Q, K and V")
    _refuse_fp8_grad("subgraph_attention", Q=Q, K=K, V=V)
    d, dv = Q.shape[1] // heads, V.shape[1] // heads
    scale = float(d) ** -0.5 if scale is None else float(scale)
    out = direction == "out"
    scores = subgraph_sddmm(engine, Q, K, heads=heads) if out else subgraph_sddmm(engine, K, Q, heads=heads)
    y = subgraph_edge_softmax(engine, scores, scale=scale, by="row" if out else "col")
    return torch.cat([subgraph_propagate_values(engine, V[:, h * dv:(h + 1) * dv], y[h], direction=direction) for h in range(heads)], dim=1)


class _SubgraphAttentionFused(torch.autograd.Function):
    """out = attention over the held subgraph in one call (Engine.subgraph_attention), y32 saved; the backward pass with the
    existing calls on it: dV = the opposite product with y[h] as values, dy = subgraph_sddmm of (G, V) -- (V, G) inwards -- and
    ds = subgraph_softmax_bwd for all heads at once, dQ and dK the two products with ds[h] as values"""

    @staticmethod
    def forward(ctx, Q, K, V, engine, scale, heads, inwards):
        out32, _, y32, _, _ = engine.subgraph_attention(Q.detach(), K.detach(), V.detach(), heads=heads, scale=scale, by="col" if inwards else "row",
                                                        want32=True, want64=False, want_y32=True)
        ctx.save_for_backward(Q, K, V, y32)
        ctx.engine, ctx.scale, ctx.heads, ctx.inwards = engine, scale, heads, inwards
        ctx.generation = engine.get_option("sparse_generation")
        return out32

    @staticmethod
    def backward(ctx, G):
        Q, K, V, y32 = ctx.saved_tensors
        engine, heads, inwards = ctx.engine, ctx.heads, ctx.inwards
        _held_guard(ctx.generation, engine, "subgraph_attention_fused")
        G = _dense_operand(G)
        d, dv = Q.shape[1] // heads, V.shape[1] // heads
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        Qd, Kd, Vd = Q.detach(), K.detach(), V.detach()
        # along: the product that sums over the forward pass's groups; across: its transpose
        along, across = (engine.subgraph_propagate_t, engine.subgraph_propagate) if inwards else (engine.subgraph_propagate, engine.subgraph_propagate_t)
        new = lambda X: torch.empty(X.shape, dtype=torch.float32, device=X.device)
        dQ, dK, dV = new(Q) if need_q else None, new(K) if need_k else None, new(V) if need_v else None
        if need_v:
            for h in range(heads):
                vs = slice(h * dv, (h + 1) * dv)
                across(G[:, vs], values=y32[h], want64=False, out32=dV[:, vs])
        if need_q or need_k:
            dy, _, _ = engine.subgraph_sddmm(Vd, G, heads=heads) if inwards else engine.subgraph_sddmm(G, Vd, heads=heads)
            ds, _, _ = engine.subgraph_softmax_bwd(y32, dy, scale=ctx.scale, by="col" if inwards else "row")
            for h in range(heads):
                qs = slice(h * d, (h + 1) * d)
                if need_q:
                    along(Kd[:, qs], values=ds[h], want64=False, out32=dQ[:, qs])
                if need_k:
                    across(Qd[:, qs], values=ds[h], want64=False, out32=dK[:, qs])
        cast = lambda g, X: g if g is None or X.dtype == torch.float32 else g.to(X.dtype)
        return cast(dQ, Q), cast(dK, K), cast(dV, V), None, None, None, None


def subgraph_attention_fused(engine, Q, K, V, heads=1, scale=None, direction="out"):
    """subgraph_attention with the forward pass in ONE library call (Engine.subgraph_attention, the EDGE ATTENTION contract): a
    node's edges are scored, normalised and multiplied by one wave for up to four heads at a time, nothing is written between
    the steps and nothing is rounded to float32 between them.  Operands, direction, scale and the result as for
    subgraph_attention: Q, K [nc, heads * d], V [nc, heads * dv], float32, bfloat16 or float16 tensors on the engine's GPU (FP8
    as constants); float32 [nc, heads * dv], differentiable in Q, K and V.  The backward pass runs the existing calls on the
    float32 probabilities the forward call saved: the scores' and the softmax's gradients for all heads in one call each, the
    products head by head.  The subgraph must still be held when it runs."""
    heads = int(heads)
    if direction not in ("out", "in"):
        raise ValueError('subgraph_attention_fused: direction is "out" or "in"')
    if heads < 1 or Q.dim() != 2 or K.dim() != 2 or V.dim() != 2 or Q.shape[1] % heads or V.shape[1] % heads or K.shape[1] != Q.shape[1]:
        raise ValueError("subgraph_attention_fused: heads must be at least 1 and divide the columns of Q, K and V, and Q and K be as wide")
    _refuse_fp8_grad("subgraph_attention_fused", Q=Q, K=K, V=V)
    scale = float(Q.shape[1] // heads) ** -0.5 if scale is None else float(scale)
    return _SubgraphAttentionFused.apply(Q, K, V, engine, scale, heads, direction == "in")


class _SubgraphAttentionTrained(_SubgraphAttentionFused):
    """the same forward pass; the backward pass is ONE call for all heads (Engine.subgraph_attention_bwd) on the saved y32, with
    nothing rounded to float32 between its steps"""

    @staticmethod
    def backward(ctx, G):
        Q, K, V, y32 = ctx.saved_tensors
        engine = ctx.engine
        _held_guard(ctx.generation, engine, "subgraph_attention_trained")
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        if not (need_q or need_k or need_v):
            return None, None, None, None, None, None, None
        dQ, _, dK, _, dV, _, stats = engine.subgraph_attention_bwd(Q.detach(), K.detach(), V.detach(), _dense_operand(G), y32, heads=ctx.heads, scale=ctx.scale,
                                                                   by="col" if ctx.inwards else "row", want_dq=need_q, want_dk=need_k, want_dv=need_v,
                                                                   want32=True, want64=False)
        engine.last_subgraph_attention_bwd = stats
        cast = lambda g, X: g if g is None or X.dtype == torch.float32 else g.to(X.dtype)
        return cast(dQ, Q), cast(dK, K), cast(dV, V), None, None, None, None


def subgraph_attention_trained(engine, Q, K, V, heads=1, scale=None, direction="out"):
    """subgraph_attention_fused with the backward pass in ONE library call as well (Engine.subgraph_attention_bwd, the EDGE
    ATTENTION, BACKWARD contract): the same forward call and result, the float32 probabilities saved; the backward pass computes
    only the gradients autograd asks for, for all heads at once, and rounds nothing to float32 between its steps -- a layer's
    training step is two library calls.  Operands, heads, scale and direction as for subgraph_attention_fused.  The subgraph
    must still be held when the backward pass runs; its stats are left in engine.last_subgraph_attention_bwd."""
    heads = int(heads)
    if direction not in ("out", "in"):
        raise ValueError('subgraph_attention_trained: direction is "out" or "in"')
    if heads < 1 or Q.dim() != 2 or K.dim() != 2 or V.dim() != 2 or Q.shape[1] % heads or V.shape[1] % heads or K.shape[1] != Q.shape[1]:
        raise ValueError("subgraph_attention_trained: heads must be at least 1 and divide the columns of Q, K and V, and Q and K be as wide")
    _refuse_fp8_grad("subgraph_attention_trained", Q=Q, K=K, V=V)
    scale = float(Q.shape[1] // heads) ** -0.5 if scale is None else float(scale)
    return _SubgraphAttentionTrained.apply(Q, K, V, engine, scale, heads, direction == "in")


class _SubgraphGat(torch.autograd.Function):
    """out = graph attention over the held subgraph in one call (Engine.subgraph_gat), y32 saved; the backward pass is ONE call
    for all heads (Engine.subgraph_gat_bwd) on it, for the gradients autograd asks for"""

    @staticmethod
    def forward(ctx, el, er, V, engine, slope, heads, inwards):
        out32, _, y32, _, _ = engine.subgraph_gat(el.detach(), er.detach(), V.detach(), heads=heads, slope=slope, by="col" if inwards else "row",
                                                  want32=True, want64=False, want_y32=True)
        ctx.save_for_backward(el, er, V, y32)
        ctx.engine, ctx.slope, ctx.heads, ctx.inwards = engine, slope, heads, inwards
        ctx.generation = engine.get_option("sparse_generation")
        return out32

    @staticmethod
    def backward(ctx, G):
        el, er, V, y32 = ctx.saved_tensors
        engine = ctx.engine
        _held_guard(ctx.generation, engine, "subgraph_gat")
        need_l, need_r, need_v = ctx.needs_input_grad[:3]
        if not (need_l or need_r or need_v):
            return None, None, None, None, None, None, None
        dl, _, dr, _, dV, _, stats = engine.subgraph_gat_bwd(el.detach(), er.detach(), V.detach(), _dense_operand(G), y32, heads=ctx.heads, slope=ctx.slope,
                                                             by="col" if ctx.inwards else "row", want_del=need_l, want_der=need_r, want_dv=need_v,
                                                             want32=True, want64=False)
        engine.last_subgraph_gat_bwd = stats
        cast = lambda g, X: g if g is None or X.dtype == torch.float32 else g.to(X.dtype)
        return cast(dl, el), cast(dr, er), cast(dV, V), None, None, None, None


def subgraph_gat(engine, el, er, V, heads=1, slope=0.2, direction="out"):
    """A graph attention network's layer over the sampled graph in two library calls (Engine.subgraph_gat and, backward,
    Engine.subgraph_gat_bwd; the EDGE GAT contracts): the score of edge e is LeakyReLU(el[row of e] + er[sub_col[e]]) with the
    negative slope `slope`, per head -- el = (feat * attn_l).sum(-1) and er = (feat * attn_r).sum(-1) of a GATConv layer.
    direction="out": node j attends over its out-edges, out[j] = sum over the edges e of row j of y[e] * V[sub_col[e]];
    direction="in": node v over its in-edges, out[v] = sum over the edges e with sub_col[e] == v of y[e] * V[row of e]; y the
    softmax of the scores over the node's edges.  el, er: [nc, heads], V: [nc, heads * dv], float32, bfloat16 or float16
    tensors on the engine's GPU (FP8 as constants).  Returns float32 [nc, heads * dv], differentiable in el, er and V; nothing
    is rounded to float32 between the steps of either pass.  The subgraph must still be held when the backward pass runs; its
    stats are left in engine.last_subgraph_gat_bwd."""
    heads = int(heads)
    if direction not in ("out", "in"):
        raise ValueError('subgraph_gat: direction is "out" or "in"')
    if heads < 1 or el.dim() != 2 or er.dim() != 2 or V.dim() != 2 or el.shape[1] != heads or er.shape[1] != heads or V.shape[1] % heads:
        raise ValueError("subgraph_gat: el and er must be [nc, heads] and heads (at least 1) divide the columns of V")
    _refuse_fp8_grad("subgraph_gat", el=el, er=er, V=V)
    return _SubgraphGat.apply(el, er, V, engine, float(slope), heads, direction == "in")


class _SubgraphGatv2(torch.autograd.Function):
    """out = GATv2 attention over the held subgraph in one call (Engine.subgraph_gatv2), y32 saved; the backward pass with the
    existing calls on it -- dV = the opposite product with y[h] as values, dy = subgraph_sddmm of (G, V) -- (V, G) inwards -- and
    ds = subgraph_softmax_bwd for all heads at once -- and from ds in plain torch on the edge index, head by head, so that the
    intermediate stays [edges, d]"""

    @staticmethod
    def forward(ctx, xl, xr, att, V, engine, slope, heads, inwards):
        out32, _, y32, _, _ = engine.subgraph_gatv2(xl.detach(), xr.detach(), att.detach(), V.detach(), heads=heads, slope=slope, by="col" if inwards else "row",
                                                    want32=True, want64=False, want_y32=True)
        ctx.save_for_backward(xl, xr, att, V, y32)
        ctx.engine, ctx.slope, ctx.heads, ctx.inwards = engine, slope, heads, inwards
        ctx.generation = engine.get_option("sparse_generation")
        return out32

    @staticmethod
    def backward(ctx, G):
        xl, xr, att, V, y32 = ctx.saved_tensors
        engine, heads, slope, inwards = ctx.engine, ctx.heads, ctx.slope, ctx.inwards
        _held_guard(ctx.generation, engine, "subgraph_gatv2")
        need_l, need_r, need_a, need_v = ctx.needs_input_grad[:4]
        G = _dense_operand(G)
        d, dv = xl.shape[1] // heads, V.shape[1] // heads
        f32 = lambda X: X.detach().to(torch.float32)
        dxl, dxr, datt, dV = (torch.zeros(X.shape, dtype=torch.float32, device=X.device) if need else None
                              for X, need in ((xl, need_l), (xr, need_r), (att, need_a), (V, need_v)))
        if need_v:
            across = engine.subgraph_propagate if inwards else engine.subgraph_propagate_t
            for h in range(heads):
                vs = slice(h * dv, (h + 1) * dv)
                across(G[:, vs], values=y32[h], want64=False, out32=dV[:, vs])
        if need_l or need_r or need_a:
            Vd = V.detach()
            dy, _, _ = engine.subgraph_sddmm(Vd, G, heads=heads) if inwards else engine.subgraph_sddmm(G, Vd, heads=heads)
            ds, _, _ = engine.subgraph_softmax_bwd(y32, dy, scale=1.0, by="col" if inwards else "row")
            # the edge index in the order of sub_col, from the transposition: entry p of column u is edge in_pos[p] of row in_row[p]
            in_ptr, in_row, in_pos = engine.subgraph_transpose_fetch(device=True)
            rows, cols = torch.empty_like(in_pos), torch.empty_like(in_pos)
            rows[in_pos] = in_row.to(torch.int64)
            cols[in_pos] = torch.repeat_interleave(torch.arange(in_ptr.numel() - 1, device=in_ptr.device), in_ptr[1:] - in_ptr[:-1])
            xl32, xr32, att32 = f32(xl), f32(xr), f32(att)
            for h in range(heads):
                hs = slice(h * d, (h + 1) * d)
                u = xl32[rows, hs] + xr32[cols, hs]
                dsh = ds[h].unsqueeze(1)
                if need_a:
                    datt[h] = (dsh * torch.nn.functional.leaky_relu(u, slope)).sum(0)
                if need_l or need_r:
                    du = dsh * att32[h] * torch.where(u >= 0, 1.0, slope)
                    if need_l:
                        dxl[:, hs].index_add_(0, rows, du)
                    if need_r:
                        dxr[:, hs].index_add_(0, cols, du)
        cast = lambda g, X: g if g is None or X.dtype == torch.float32 else g.to(X.dtype)
        return cast(dxl, xl), cast(dxr, xr), cast(datt, att), cast(dV, V), None, None, None, None


def subgraph_gatv2(engine, xl, xr, att, V, heads=1, slope=0.2, direction="out"):
    """A GATv2 layer over the sampled graph with the forward pass in ONE library call (Engine.subgraph_gatv2, the EDGE GATV2
    contract): the score of edge e is sum_c att[h, c] * LeakyReLU(xl[row of e, h d + c] + xr[sub_col[e], h d + c]) with the
    negative slope `slope`, per head -- xl = lin_l(x) and xr = lin_r(x) of a GATv2Conv layer; they may be one tensor.
    direction="out": node j attends over its out-edges, out[j] = sum over the edges e of row j of y[e] * V[sub_col[e]];
    direction="in": node v over its in-edges, out[v] = sum over the edges e with sub_col[e] == v of y[e] * V[row of e]; y the
    softmax of the scores over the node's edges.  xl, xr: [nc, heads * d], att: [heads, d], V: [nc, heads * dv], float32,
    bfloat16 or float16 tensors on the engine's GPU (FP8 as constants).  Returns float32 [nc, heads * dv], differentiable in xl,
    xr, att and V.  The forward pass has the contract's bits.  The backward pass is composed: the gradients of V, of the
    probabilities and of the scores come from the existing calls on the float32 probabilities the forward call saved, and the
    gradients of xl, xr and att from them in plain torch (index_add over the edge index, float32) -- this half defines no bits.
    The subgraph must still be held when it runs."""
    heads = int(heads)
    if direction not in ("out", "in"):
        raise ValueError('subgraph_gatv2: direction is "out" or "in"')
    if heads < 1 or xl.dim() != 2 or xr.dim() != 2 or V.dim() != 2 or xl.shape[1] % heads or V.shape[1] % heads or xr.shape[1] != xl.shape[1]:
        raise ValueError("subgraph_gatv2: heads must be at least 1 and divide the columns of xl, xr and V, and xl and xr be as wide")
    if att.dim() != 2 or tuple(att.shape) != (heads, xl.shape[1] // heads):
        raise ValueError("subgraph_gatv2: att must be [heads, d]")
    _refuse_fp8_grad("subgraph_gatv2", xl=xl, xr=xr, att=att, V=V)
    return _SubgraphGatv2.apply(xl, xr, att, V, engine, float(slope), heads, direction == "in")


class _SubgraphGatv2Trained(_SubgraphGatv2):
    """the same forward pass; the backward pass is ONE call for all heads (Engine.subgraph_gatv2_bwd) on the saved y32, for the
    gradients autograd asks for: float64 throughout, no atomics, the same bits on every run"""

    @staticmethod
    def backward(ctx, G):
        xl, xr, att, V, y32 = ctx.saved_tensors
        engine = ctx.engine
        _held_guard(ctx.generation, engine, "subgraph_gatv2_trained")
        need_l, need_r, need_a, need_v = ctx.needs_input_grad[:4]
        if not (need_l or need_r or need_a or need_v):
            return None, None, None, None, None, None, None, None
        dxl, _, dxr, _, datt, _, dV, _, stats = engine.subgraph_gatv2_bwd(xl.detach(), xr.detach(), att.detach(), V.detach(), _dense_operand(G), y32, heads=ctx.heads,
                                                                          slope=ctx.slope, by="col" if ctx.inwards else "row", want_dxl=need_l, want_dxr=need_r,
                                                                          want_datt=need_a, want_dv=need_v, want32=True, want64=False)
        engine.last_subgraph_gatv2_bwd = stats
        cast = lambda g, X: g if g is None or X.dtype == torch.float32 else g.to(X.dtype)
        return cast(dxl, xl), cast(dxr, xr), cast(datt, att), cast(dV, V), None, None, None, None


def subgraph_gatv2_trained(engine, xl, xr, att, V, heads=1, slope=0.2, direction="out"):
    """subgraph_gatv2 with the backward pass in ONE library call as well (Engine.subgraph_gatv2_bwd, the EDGE GATV2, BACKWARD
    contract): the same forward call and result, the float32 probabilities saved; the backward pass computes only the gradients
    autograd asks for, for all heads at once, chains them through float64 and adds every sum in a fixed order -- two runs give the
    same bits, which the composed pass of subgraph_gatv2 cannot promise.  Operands, heads, slope and direction as for
    subgraph_gatv2.  The subgraph must still be held when the backward pass runs; its stats are left in
    engine.last_subgraph_gatv2_bwd."""
    heads = int(heads)
    if direction not in ("out", "in"):
        raise ValueError('subgraph_gatv2_trained: direction is "out" or "in"')
    if heads < 1 or xl.dim() != 2 or xr.dim() != 2 or V.dim() != 2 or xl.shape[1] % heads or V.shape[1] % heads or xr.shape[1] != xl.shape[1]:
        raise ValueError("subgraph_gatv2_trained: heads must be at least 1 and divide the columns of xl, xr and V, and xl and xr be as wide")
    if att.dim() != 2 or tuple(att.shape) != (heads, xl.shape[1] // heads):
        raise ValueError("subgraph_gatv2_trained: att must be [heads, d]")
    _refuse_fp8_grad("subgraph_gatv2_trained", xl=xl, xr=xr, att=att, V=V)
    return _SubgraphGatv2Trained.apply(xl, xr, att, V, engine, float(slope), heads, direction == "in")


def ppr_sddmm(engine, row_ptr, A, B):
    """scores[e] = <A[row of e], B[id of e]> for every held entry e of `engine` (Engine.sparse_sddmm), float32 [entries] on
    the device, differentiable in A ([nq, d]) and B ([n, d], n = engine.held_cols), float32, bfloat16 or float16 tensors (or constant FP8 ones) on the engine's GPU with a column
    stride of one element: A.grad = P(g) x B and B.grad = P(g)^T x A, the two products with the scores' gradient g as values.
    The rows must still be held when the backward pass runs."""
    _refuse_fp8_grad("ppr_sddmm", A=A, B=B)
    return _PprSddmm.apply(A, B, engine, row_ptr)


def row_softmax(row_ptr, scores):
    """softmax of `scores` ([entries]) inside every row of row_ptr ([nq + 1], numpy or a tensor): per row the max is
    subtracted, then exp, then the division by the row's sum.  Plain torch (scatter operations), differentiable, on the CPU
    or on a GPU; empty rows are allowed, and nothing here has defined bits."""
    if not torch.is_tensor(row_ptr):
        row_ptr = torch.as_tensor(row_ptr)
    row_ptr = row_ptr.to(device=scores.device, dtype=torch.int64)
    nq = row_ptr.numel() - 1
    lens = row_ptr[1:] - row_ptr[:-1]
    row = torch.repeat_interleave(torch.arange(nq, device=scores.device), lens, output_size=scores.numel())
    top = torch.full((nq,), float("-inf"), dtype=scores.dtype, device=scores.device)
    top = top.scatter_reduce(0, row, scores.detach(), reduce="amax", include_self=True)
    ex = torch.exp(scores - top[row])
    den = torch.zeros(nq, dtype=scores.dtype, device=scores.device).index_add(0, row, ex)
    return ex / den[row]


class _PprRowSoftmax(torch.autograd.Function):
    """y = softmax_row(scores * scale) (Engine.sparse_softmax): dscores = ((g - sum_row(y g)) y) scale (Engine.sparse_softmax_bwd)"""

    @staticmethod
    def forward(ctx, scores, engine, row_ptr, scale):
        s = scores.detach()
        if s.dtype not in (torch.float32, torch.float64):
            s = s.to(torch.float32)
        y32, _, _ = engine.sparse_softmax(row_ptr, s, scale=scale, want32=True, want64=False)
        ctx.save_for_backward(y32)
        ctx.engine, ctx.row_ptr, ctx.scale, ctx.dtype = engine, row_ptr, scale, scores.dtype
        ctx.generation = engine.get_option("sparse_generation")
        return y32

    @staticmethod
    def backward(ctx, g):
        (y32,) = ctx.saved_tensors
        _held_guard(ctx.generation, ctx.engine, "ppr_row_softmax")
        dx, _, _ = ctx.engine.sparse_softmax_bwd(ctx.row_ptr, y32, _entry_values(g), scale=ctx.scale, want32=True, want64=False)
        return (dx if ctx.dtype == torch.float32 else dx.to(ctx.dtype)), None, None, None


def ppr_row_softmax(engine, row_ptr, scores, scale=1.0):
    """softmax of scores * scale inside every held row of `engine` (Engine.sparse_softmax, the ROW SOFTMAX contract: a defined
    exp, a fixed order, every bit defined), float32 [entries] on the device, differentiable in scores (a float32 or float64
    tensor of one element per held entry on the engine's GPU; the gradient comes back in its dtype).  The backward pass is
    Engine.sparse_softmax_bwd on the saved float32 output.  scale is a number, not a differentiable operand: a learned
    temperature multiplies the scores before the call.  The rows must still be held when the backward pass runs."""
    return _PprRowSoftmax.apply(scores, engine, row_ptr, float(scale))


class _PprAttentionFused(torch.autograd.Function):
    """out = attention over the held rows in one call (Engine.sparse_attention), y32 saved; the backward pass head by head on
    column slices with the existing calls: dV = P(y)^T x G, dy = sddmm(G, V), ds = softmax_bwd(y, dy), dQ = P(ds) x K,
    dK = P(ds)^T x Q"""

    @staticmethod
    def forward(ctx, Q, K, V, engine, row_ptr, scale, heads):
        out32, _, y32, _, _ = engine.sparse_attention(row_ptr, Q.detach(), K.detach(), V.detach(), heads=heads, scale=scale,
                                                      want32=True, want64=False, want_y32=True)
        ctx.save_for_backward(Q, K, V, y32)
        ctx.engine, ctx.row_ptr, ctx.scale, ctx.heads = engine, row_ptr, scale, heads
        ctx.generation = engine.get_option("sparse_generation")
        return out32

    @staticmethod
    def backward(ctx, G):
        Q, K, V, y32 = ctx.saved_tensors
        engine, row_ptr, heads = ctx.engine, ctx.row_ptr, ctx.heads
        _held_guard(ctx.generation, engine, "ppr_attention_fused")
        G = _dense_operand(G)
        d, dv = Q.shape[1] // heads, V.shape[1] // heads
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        Qd, Kd, Vd = Q.detach(), K.detach(), V.detach()
        dQ = torch.empty(Q.shape, dtype=torch.float32, device=Q.device) if need_q else None
        dK = torch.empty(K.shape, dtype=torch.float32, device=K.device) if need_k else None
        dV = torch.empty(V.shape, dtype=torch.float32, device=V.device) if need_v else None
        for j in range(heads):
            qs, vs = slice(j * d, (j + 1) * d), slice(j * dv, (j + 1) * dv)
            Gj, yj = G[:, vs], y32[j]
            if need_v:
                engine.sparse_propagate_t(row_ptr, Gj, want64=False, values=yj, out32=dV[:, vs])
            if need_q or need_k:
                dy, _, _ = engine.sparse_sddmm(row_ptr, Gj, Vd[:, vs], want32=True, want64=False)
                ds, _, _ = engine.sparse_softmax_bwd(row_ptr, yj, dy, scale=ctx.scale, want32=True, want64=False)
                if need_q:
                    engine.sparse_propagate(row_ptr, Kd[:, qs], want64=False, values=ds, out32=dQ[:, qs])
                if need_k:
                    engine.sparse_propagate_t(row_ptr, Qd[:, qs], want64=False, values=ds, out32=dK[:, qs])
        cast = lambda g, X: g if g is None or X.dtype == torch.float32 else g.to(X.dtype)
        return cast(dQ, Q), cast(dK, K), cast(dV, V), None, None, None, None


class _PprAttentionFusedBwd(_PprAttentionFused):
    """the same forward pass; the backward pass is ONE call for all heads (Engine.sparse_attention_bwd) on the saved y32, with
    nothing rounded to float32 between its steps"""

    @staticmethod
    def backward(ctx, G):
        Q, K, V, y32 = ctx.saved_tensors
        engine = ctx.engine
        _held_guard(ctx.generation, engine, "ppr_attention_fused")
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        if not (need_q or need_k or need_v):
            return None, None, None, None, None, None, None
        dQ, _, dK, _, dV, _, _ = engine.sparse_attention_bwd(ctx.row_ptr, Q.detach(), K.detach(), V.detach(), _dense_operand(G), y32, heads=ctx.heads,
                                                             scale=ctx.scale, want_dq=need_q, want_dk=need_k, want_dv=need_v, want32=True, want64=False)
        cast = lambda g, X: g if g is None or X.dtype == torch.float32 else g.to(X.dtype)
        return cast(dQ, Q), cast(dK, K), cast(dV, V), None, None, None, None


def ppr_attention_fused(engine, row_ptr, Q, K, V, scale=None, heads=1, backward="calls"):
    """ppr_attention with all three steps in ONE library call (Engine.sparse_attention, the ATTENTION contract): the rows of at
    most 256 entries are scored, normalised and multiplied by one wave each without anything written in between, and nothing
    is rounded to float32 between the steps.  Q: [nq, heads * d], K: [n, heads * d], V: [n, heads * dv] (n =
    engine.held_cols: over a compacted result K and V are the rows `cols` of the full matrices), float32, bfloat16 or float16 (or constant FP8 tensors) on the
    engine's GPU; head j attends with the columns [j * d, (j + 1) * d) of Q and K and writes the columns
    [j * dv, (j + 1) * dv) of the result, [nq, heads * dv] float32.  scale defaults to d ** -0.5 and is a number, not a
    differentiable operand.  Differentiable in Q, K and V: the backward pass runs head by head with the calls ppr_attention
    (softmax="engine") uses, on the float32 probabilities the forward call saved.  The rows must still be held when it runs.
    backward: "calls" (the default) is that head-by-head pass; "fused" makes the backward pass one library call for all heads
    (Engine.sparse_attention_bwd, the ATTENTION, BACKWARD contract) on the same saved probabilities, computing only the
    gradients autograd asks for and rounding nothing to float32 between its steps."""
    heads = int(heads)
    if heads < 1 or Q.shape[1] % heads or V.shape[1] % heads:
        raise ValueError("ppr_attention_fused: heads must be at least 1 and divide the columns of Q and of V")
    if backward not in ("calls", "fused"):
        raise ValueError('ppr_attention_fused: backward is "calls" or "fused"')
    _refuse_fp8_grad("ppr_attention_fused", Q=Q, K=K, V=V)
    if scale is None:
        scale = float(Q.shape[1] // heads) ** -0.5
    fn = _PprAttentionFused if backward == "calls" else _PprAttentionFusedBwd
    return fn.apply(Q, K, V, engine, row_ptr, float(scale), heads)


def ppr_attention(engine, row_ptr, Q, K, V, scale=None, softmax="torch"):
    """Attention of every row over its held neighbourhood: out[i] = sum over the entries e of row i of
    softmax_row(scale * <Q[i], K[id_e]>)_e * V[id_e] -- ppr_propagate(V, values=row_softmax(ppr_sddmm(Q, K) * scale)).
    Q: [nq, d], K: [n, d], V: [n, dv] (n = engine.held_cols); scale defaults to d ** -0.5.  Differentiable in Q, K and V.
    softmax: "torch" (the default) takes the softmax with row_softmax, plain torch; "engine" with ppr_row_softmax, scale
    folded into the call -- all three steps in the library, forward and backward, every bit defined; "fused" is
    ppr_attention_fused with one head -- the forward pass in one library call."""
    if scale is None:
        scale = float(Q.shape[1]) ** -0.5
    if softmax == "fused":
        return ppr_attention_fused(engine, row_ptr, Q, K, V, scale=scale, heads=1)
    scores = ppr_sddmm(engine, row_ptr, Q, K)
    if softmax == "engine":
        return ppr_propagate(engine, row_ptr, V, values=ppr_row_softmax(engine, row_ptr, scores, scale))
    if softmax != "torch":
        raise ValueError('ppr_attention: softmax is "torch", "engine" or "fused"')
    return ppr_propagate(engine, row_ptr, V, values=row_softmax(row_ptr, scores * scale))
