"""The batch-norm layer of a conv -> SyncBN -> activation block on the fused HIP path, as ``FusedNecks`` and ``FCNHead`` use it:
the SyncBN exchange, the batch vectors with nn.SyncBatchNorm's bookkeeping, the tail of the backward, and the per-shape buffer
cache.  Pure torch plumbing on tiny vectors; the kernels that make the sums are the caller's (csrc/bn_tile.hpp has their
shared device pieces)."""
import torch


def all_reduce_sum(vec, tag):
    """Sum ``vec`` over the ranks when torch.distributed runs with more than one; ``tag`` is "stats" (the [count, sum,
    sum of squares] rows of the batch statistics) or "bwd" (the [sum g, sum g xhat] rows of the batch-norm backward).  Both
    are tiny.  ``FusedNecks.reduce`` and ``FCNHead.reduce`` hold this function; a test replaces it."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(vec)
    return vec


def batch_vectors(bn, stats, reduce, shift=None):
    """(mean, rstd, 1 / n) of the batch norm ``bn``: the batch statistics in train() over the n elements per channel of every
    rank (running statistics updated as nn.SyncBatchNorm does: momentum, unbiased variance, num_batches_tracked), the running
    ones in eval() (no n; neither ``stats`` nor ``reduce`` is called).  ``stats()`` -> f32 [3, C]: count, sum (x - shift),
    sum (x - shift)^2 of this rank; ``shift`` [C] is what the sums were shifted by, None: nothing."""
    if not bn.training:
        return bn.running_mean.contiguous(), torch.rsqrt(bn.running_var + bn.eps), None
    st = reduce(stats(), "stats")
    n = st[0]
    m1 = st[1] / n
    mean = m1 if shift is None else shift + m1
    var = (st[2] / n - m1 * m1).clamp_(min=0.0)
    with torch.no_grad():
        assert bn.momentum is not None, "the batch norm %r has momentum 0.1 (no cumulative average)" % (bn,)
        bn.running_mean.mul_(1.0 - bn.momentum).add_(mean, alpha=bn.momentum)
        bn.running_var.mul_(1.0 - bn.momentum).add_(var * (n / (n - 1.0)), alpha=bn.momentum)
        bn.num_batches_tracked += 1
    return mean, torch.rsqrt(var + bn.eps), 1.0 / n


def batch_vectors_stacked(bns, stats, reduce):
    """``batch_vectors`` for several batch norms of one width whose statistics travel in ONE exchange (the pyramid branches of
    ``PSPHead``): ``stats()`` -> f32 [len(bns), 3, C], unshifted, one ``reduce(., "stats")`` for all of them.  Returns (mean
    [n, C], rstd [n, C], 1 / n [n, C]); the arithmetic and the bookkeeping per batch norm are ``batch_vectors``'s.  eval(): the
    running statistics, no 1 / n; neither ``stats`` nor ``reduce`` is called."""
    if not bns[0].training:
        return (torch.stack([bn.running_mean for bn in bns]), torch.stack([torch.rsqrt(bn.running_var + bn.eps) for bn in bns]), None)
    st = reduce(stats(), "stats")
    n = st[:, 0]
    mean = st[:, 1] / n
    var = (st[:, 2] / n - mean * mean).clamp_(min=0.0)
    with torch.no_grad():
        for i, bn in enumerate(bns):
            assert bn.momentum is not None, "the batch norm %r has momentum 0.1 (no cumulative average)" % (bn,)
            bn.running_mean.mul_(1.0 - bn.momentum).add_(mean[i], alpha=bn.momentum)
            bn.running_var.mul_(1.0 - bn.momentum).add_(var[i] * (n[i] / (n[i] - 1.0)), alpha=bn.momentum)
            bn.num_batches_tracked += 1
    return mean, torch.stack([torch.rsqrt(var[i] + bn.eps) for i, bn in enumerate(bns)]), 1.0 / n


def grad_of(p):
    """``p.grad``, zeros at first use: the backward walks accumulate into it themselves."""
    if p.grad is None:
        p.grad = torch.zeros_like(p)
    return p.grad


def add_affine_grads(bn, sums):
    """The rows of ``sums`` [2, C] = sum g, sum g xhat of this rank are the gradients of ``bn.bias`` and ``bn.weight``."""
    if bn.bias.requires_grad:
        grad_of(bn.bias).add_(sums[0])
    if bn.weight.requires_grad:
        grad_of(bn.weight).add_(sums[1])


def backward_totals(sums, inv_n, reduce):
    """The two sums over every rank, divided on the device by the element count the forward's statistics had (no read-back);
    None with eval statistics (``inv_n`` None: no correction terms)."""
    return None if inv_n is None else (reduce(sums.clone(), "bwd") * inv_n).contiguous()


class BufferCache:
    """Buffers per (name, shape, dtype), allocated once on ``_buf_device()`` and reused."""

    def _buf_device(self):
        raise NotImplementedError

    def _buf(self, name, shape, dtype=torch.bfloat16, zero=False):
        key = (name, tuple(shape), dtype)
        b = self._bufs.get(key)
        if b is None:
            make = torch.zeros if zero else torch.empty
            b = self._bufs[key] = make(shape, dtype=dtype, device=self._buf_device())
        return b

    _grad = staticmethod(grad_of)
