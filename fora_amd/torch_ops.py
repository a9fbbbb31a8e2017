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
A_S^T x X, each the other's gradient."""
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
    gradient is an SDDMM over the subgraph's edges, which the library does not have yet).
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
                             "(its gradient is an SDDMM over the subgraph's edges)")
        values = _entry_values(values.detach())
    if norm == "mean" and values is not None:
        raise ValueError("subgraph_propagate: norm and values exclude each other (pass the normalisation as values)")
    return _SubgraphPropagate.apply(X, engine, values, norm == "mean", direction == "in")


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
