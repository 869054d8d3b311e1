"""-m "not gpu": mem_amd.syncbn, the batch-norm plumbing FusedNecks and FCNHead share -- the batch vectors and the bookkeeping
against a float64 nn.BatchNorm2d, the tail of the backward, the one SyncBN exchange, the buffer cache."""
import pytest
import torch
import torch.nn as nn

N = 12                    # elements per channel
BAR = 1e-5                # relative L2 per vector: the bar tests/test_necks_gpu.py holds the same arithmetic to


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _data(C, seed):
    """float64 [N, C] with |mean| <= std per channel, so that E[x^2] - m1^2 does not cancel"""
    gen = torch.Generator().manual_seed(seed)
    std = 1.0 + torch.rand(C, generator=gen, dtype=torch.float64)
    mean = (2.0 * torch.rand(C, generator=gen, dtype=torch.float64) - 1.0) * std
    return torch.randn(N, C, generator=gen, dtype=torch.float64) * std + mean


def _fake_stats(x, shift, calls):
    """the [3, C] tensor a stats kernel returns: count, sum (x - shift), sum (x - shift)^2, float64 sums cast to fp32"""
    def stats():
        calls.append("stats")
        d = x - (0.0 if shift is None else shift.double())
        return torch.stack([torch.full((x.shape[1],), float(x.shape[0]), dtype=torch.float64), d.sum(0), (d * d).sum(0)]).float()
    return stats


def _recording_reduce(tags):
    def reduce(vec, tag):
        tags.append(tag)
        return vec
    return reduce


@pytest.mark.parametrize("C", [1, 5])
def test_batch_vectors_against_float64_batchnorm(C):
    from mem_amd.syncbn import batch_vectors
    ref = nn.BatchNorm2d(C).double().train()
    plain, shifted = nn.BatchNorm2d(C).train(), nn.BatchNorm2d(C).train()
    shift = torch.tensor([0.25, -0.5, 1.0, 0.0, -1.5][:C])
    for call in (1, 2):
        x = _data(C, seed=10 * C + call)
        ref(x.reshape(N, C, 1, 1))
        want_mean, want_var = x.mean(0), x.var(0, unbiased=False)
        got = []
        for bn, s in ((plain, None), (shifted, shift)):
            tags, calls = [], []
            stats = _fake_stats(x, s, calls)
            mean, rstd, inv_n = batch_vectors(bn, stats, _recording_reduce(tags), shift=s)
            assert tags == ["stats"] and calls == ["stats"]
            assert mean.dtype == torch.float32 and tuple(mean.shape) == (C,) and tuple(rstd.shape) == (C,)
            assert _rel(mean, want_mean) <= BAR and _rel(rstd, torch.rsqrt(want_var + bn.eps)) <= BAR
            assert torch.equal(inv_n, torch.full((C,), 1.0 / N))
            if s is None:
                st = stats()
                assert torch.equal(mean, st[1] / st[0])                   # m1 itself: no zero added
            for name in ("running_mean", "running_var"):
                rel = _rel(getattr(bn, name), getattr(ref, name))
                print("C=%d call %d %s %s rel %.3e" % (C, call, "shifted" if s is not None else "plain", name, rel))
                assert rel <= BAR, (name, rel)
            assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == call
            got.append(mean)
        assert _rel(got[1], got[0]) <= BAR


def test_batch_vectors_in_eval_calls_nothing_and_touches_nothing():
    from mem_amd.syncbn import batch_vectors
    C = 5
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.running_mean.copy_(torch.linspace(-1.0, 1.0, C))
        bn.running_var.copy_(torch.linspace(0.5, 2.0, C))
        bn.num_batches_tracked.fill_(3)
    bn.eval()
    before = {k: v.clone() for k, v in bn.state_dict().items()}

    def never(*a):
        raise AssertionError("called in eval()")

    mean, rstd, inv_n = batch_vectors(bn, never, never, shift=torch.ones(C))
    assert inv_n is None
    assert torch.equal(mean, before["running_mean"]) and torch.equal(rstd, torch.rsqrt(before["running_var"] + bn.eps))
    assert mean.is_contiguous()
    assert all(torch.equal(v, before[k]) for k, v in bn.state_dict().items())


def test_batch_vectors_refuses_a_cumulative_average():
    from mem_amd.syncbn import batch_vectors
    bn = nn.BatchNorm2d(1, momentum=None).train()
    with pytest.raises(AssertionError, match="momentum"):
        batch_vectors(bn, _fake_stats(_data(1, 0), None, []), _recording_reduce([]))


def test_backward_totals():
    from mem_amd.syncbn import backward_totals
    sums = torch.arange(10.0).reshape(2, 5)
    kept = sums.clone()

    def never(*a):
        raise AssertionError("called with eval statistics")

    assert backward_totals(sums, None, never) is None
    seen = []

    def two_ranks(vec, tag):
        seen.append((tag, vec.data_ptr()))
        return vec.mul_(2.0)                                              # in place, as an all-reduce is

    inv_n = torch.full((5,), 1.0 / N)
    tot = backward_totals(sums, inv_n, two_ranks)
    assert [t for t, _ in seen] == ["bwd"] and seen[0][1] != sums.data_ptr()
    assert torch.equal(sums, kept)
    assert torch.equal(tot, kept * 2.0 * inv_n) and tot.is_contiguous()


def test_add_affine_grads_obeys_requires_grad():
    from mem_amd.syncbn import add_affine_grads
    bn = nn.BatchNorm2d(3)
    bn.weight.requires_grad_(False)
    sums = torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    add_affine_grads(bn, sums)
    add_affine_grads(bn, sums)
    assert bn.weight.grad is None and torch.equal(bn.bias.grad, 2.0 * sums[0])
    bn.weight.requires_grad_(True)
    add_affine_grads(bn, sums)
    assert torch.equal(bn.weight.grad, sums[1]) and torch.equal(bn.bias.grad, 3.0 * sums[0])


def test_one_all_reduce_sum():
    from mem_amd import necks, seg_heads, syncbn
    assert necks.all_reduce_sum is seg_heads.all_reduce_sum is syncbn.all_reduce_sum
    v = torch.ones(3)
    assert syncbn.all_reduce_sum(v, "stats") is v                         # one rank: nothing to add


def test_buffer_cache():
    from mem_amd.syncbn import BufferCache

    class Holder(BufferCache):
        def __init__(self):
            self._bufs = {}

        def _buf_device(self):
            return torch.device("cpu")

    hd = Holder()
    a = hd._buf("a", (2, 3))
    assert a.dtype == torch.bfloat16 and tuple(a.shape) == (2, 3) and a.device.type == "cpu"
    assert hd._buf("a", [2, 3]) is a
    assert hd._buf("a", (3, 2)) is not a and hd._buf("a", (2, 3), torch.float32) is not a and hd._buf("b", (2, 3)) is not a
    assert set(hd._bufs) == {("a", (2, 3), torch.bfloat16), ("a", (3, 2), torch.bfloat16), ("a", (2, 3), torch.float32),
                             ("b", (2, 3), torch.bfloat16)}
    z = hd._buf("z", (4,), torch.float32, zero=True)
    assert torch.equal(z, torch.zeros(4))
    z.fill_(7.0)
    assert hd._buf("z", (4,), torch.float32, zero=True) is z and bool((z == 7.0).all())      # zero-filled once, at allocation
    p = nn.Parameter(torch.ones(2))
    g = hd._grad(p)
    assert torch.equal(g, torch.zeros(2)) and hd._grad(p) is g and p.grad is g
