"""torch.autograd over the held sparse rows: Z = PI * H forward (Engine.sparse_propagate), dL/dH = PI^T * dL/dZ backward
(Engine.sparse_propagate_t), both on the rows the engine holds -- the propagation step of an APPNP / PPRGo style model whose
rows are computed once and whose H = MLP(X) changes at every step.  Import torch before the first Engine is created, so that
the library and torch share one HIP runtime.  fora_amd/__init__.py does not import this module: the package needs no torch."""
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
        if G.dtype not in (torch.float32, torch.bfloat16):
            G = G.to(torch.float32)
        if G.dim() != 2 or (G.shape[1] > 1 and G.stride(1) != 1) or (G.shape[0] > 1 and G.stride(0) < G.shape[1]):
            G = G.contiguous()  # (an expanded or transposed gradient; a row-strided one is read in place)
        out32, _, _ = engine.sparse_propagate_t(ctx.row_ptr, G, normalize=ctx.normalize, want32=True, want64=False)
        return (out32 if ctx.dtype == torch.float32 else out32.to(ctx.dtype)), None, None, None


def ppr_propagate(engine, row_ptr, H, normalize=False):
    """Z = (held sparse rows of `engine`) x H as a differentiable torch operation.  row_ptr: as query_sparse /
    query_seeds_sparse returned it (a numpy array or a tensor).  H: [n, d] float32 or bfloat16 on the engine's GPU, column
    stride one element.  Returns Z [nq, d] float32 on the device; Z.backward(G) leaves H.grad = (held rows)^T x G in H's
    dtype.  The rows must still be held when the backward pass runs: a query_sparse, query_seeds_sparse, sparse_clear or
    set_graph in between makes it raise."""
    return _PprPropagate.apply(H, engine, row_ptr, bool(normalize))
