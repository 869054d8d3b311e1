"""The dVAE's training kernels on the GPU: ops.conv_wgrad (csrc/conv_wgrad.hip), ops.relu_bwd_colsum, and every data gradient
of the model through the existing forward kernels with a re-read weight (vae_model.pack_dgrad_weight).  Reference: autograd's
gradients of eventvae/vae/vae_model.py:29-41,86-102.

conv_wgrad: exact one-hot probes (big = a single 1.0: every element of G is exactly one value of small, or exactly 0, whatever
the slicing), then random layers against float64 with a DERIVED bar -- products of bf16 values are exact in fp32 and the
accumulation is fp32, so |G - G64| <= M * 2^-23 * sum |small * big| per element, the right side evaluated in float64.  The
workspace is pre-filled with NaN, small's border ring too (it is never read); big's ring is read and is zero."""
import pytest
import torch
import torch.nn.functional as F

from test_conv_wgrad_cpu import SHAPES

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _operands(shape, seed, zero_big=False):
    """(small, big) bf16 on the GPU in the kernel's formats, and (small [B, Hs, Ws, N], big_pad [B, Hbp, Wbp, C]) as float64 CPU
    views of the same values.  small's ring is NaN where it has one; big's ring is zero."""
    k, s, pad, B, Hs, Ws, C_, N, padded = shape
    g = torch.Generator().manual_seed(seed)
    sm = torch.randn(B, Hs, Ws, N, generator=g).bfloat16()
    bg = torch.zeros(B, s * Hs + 2, s * Ws + 2, C_, dtype=torch.bfloat16)
    if not zero_big:
        bg[:, 1:-1, 1:-1] = torch.randn(B, s * Hs, s * Ws, C_, generator=g).bfloat16()
    if padded:
        small = torch.full((B, Hs + 2, Ws + 2, N), NAN, dtype=torch.bfloat16)
        small[:, 1:-1, 1:-1] = sm
    else:
        small = sm.reshape(B * Hs * Ws, N).clone()
    return small.cuda(), bg.cuda(), sm.double(), bg.double()


def _workspace(shape):
    from mem_amd import ops
    k, s, pad, B, Hs, Ws, C_, N, padded = shape
    nbytes = ops.conv_wgrad_workspace(B, Hs, Ws, C_, N, k, s, pad, small_padded=bool(padded))
    return torch.full((max(nbytes // 4, 4),), NAN, dtype=torch.float32, device="cuda"), nbytes


def _run(shape, small, big, grad=None, accumulate=False):
    from mem_amd import ops
    k, s, pad, B, Hs, Ws, C_, N, padded = shape
    ws, nbytes = _workspace(shape)
    if grad is None:
        grad = torch.full((N, k * k * C_), NAN, dtype=torch.float32, device="cuda")
    ops.conv_wgrad(small, big, grad, B, Hs, Ws, C_, N, k, s, pad, small_padded=bool(padded), accumulate=accumulate,
                   workspace=ws if nbytes else None)
    return grad


def _reference(shape, sm64, bg64, absolute=False):
    """G64 [N, (ky, kx, c)] by the definition, tap by tap; absolute: sum |small * big| instead."""
    k, s, pad, B, Hs, Ws, C_, N, _ = shape
    if absolute:
        sm64, bg64 = sm64.abs(), bg64.abs()
    out = torch.zeros(N, k, k, C_, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            win = bg64[:, ky + 1 - pad: ky + 1 - pad + s * Hs: s, kx + 1 - pad: kx + 1 - pad + s * Ws: s]     # [B, Hs, Ws, C]
            out[:, ky, kx] = torch.einsum("byxn,byxc->nc", sm64, win)
    return out.reshape(N, k * k * C_)


def _probes(B, Hb, Wb, C_):
    """(b, Y, X, c) in big's interior coordinates: the four corners, the edges, the interior; b = B-1; c in both halves of a
    128-column tile and in the last chunk."""
    return [(0, 0, 0, 0), (B - 1, Hb - 1, Wb - 1, C_ - 1), (0, 0, Wb - 1, min(3, C_ - 1)), (B - 1, Hb - 1, 0, C_ // 2),
            (1 % B, 0, Wb // 2, C_ - 1), (B - 1, Hb // 2, 0, 1 % C_), (1 % B, Hb // 2, Wb // 2, (3 * C_) // 4),
            (B - 1, Hb // 2 + 1, Wb // 2 - 1, (C_ // 2 + 5) % C_)]


@pytest.mark.parametrize("name", list(SHAPES))
def test_one_hot_probes_are_exact(name):
    shape = SHAPES[name]
    k, s, pad, B, Hs, Ws, C_, N, padded = shape
    small, big, sm64, _ = _operands(shape, seed=11, zero_big=True)
    sm32 = sm64.float()
    for b, Y, X, c in _probes(B, s * Hs, s * Ws, C_):
        big[b, Y + 1, X + 1, c] = 1.0
        got = _run(shape, small, big).cpu().view(N, k, k, C_)
        big[b, Y + 1, X + 1, c] = 0.0
        want = torch.zeros(N, k, k, C_)
        for ky in range(k):
            for kx in range(k):
                ny, nx = Y + pad - ky, X + pad - kx              # s*y + ky - pad == Y
                if ny % s == 0 and nx % s == 0 and 0 <= ny // s < Hs and 0 <= nx // s < Ws:
                    want[:, ky, kx, c] = sm32[b, ny // s, nx // s]
        assert want.abs().sum() > 0
        assert torch.equal(got, want), (name, (b, Y, X, c), int((got != want).sum()), int(torch.isnan(got).sum()))


@pytest.mark.parametrize("name", list(SHAPES))
def test_random_layers_vs_float64(name):
    shape = SHAPES[name]
    k, s, pad, B, Hs, Ws, C_, N, padded = shape
    M = B * Hs * Ws
    small, big, sm64, bg64 = _operands(shape, seed=5)
    g64 = _reference(shape, sm64, bg64)
    bound = M * 2.0 ** -23 * _reference(shape, sm64, bg64, absolute=True)
    got = _run(shape, small, big)
    err = (got.cpu().double() - g64).abs()
    print(name, "max err / bound", float((err / bound.clamp_min(1e-300)).max()), "max |G|", float(g64.abs().max()))
    assert not torch.isnan(got).any()
    assert bool((err <= bound).all()), float((err - bound).max())
    # the same bits again
    assert torch.equal(_run(shape, small, big), got)
    # accumulate: onto a pre-filled G.  fl(pre + s) adds one rounding of the result: 2^-24 |pre + s| <= 2^-23 (|pre| + |G64|)
    pre = torch.randn(N, k * k * C_, generator=torch.Generator().manual_seed(9))
    acc = _run(shape, small, big, grad=pre.clone().cuda(), accumulate=True)
    err = (acc.cpu().double() - (pre.double() + g64)).abs()
    assert bool((err <= bound + 2.0 ** -23 * (pre.double().abs() + g64.abs())).all())
    assert torch.equal(_run(shape, small, big, grad=pre.clone().cuda(), accumulate=True), acc)


def test_workspace_too_small_is_refused():
    from mem_amd import _lib, ops
    shape = SHAPES["3x3_many_slices"]
    k, s, pad, B, Hs, Ws, C_, N, padded = shape
    small, big, _, _ = _operands(shape, seed=1)
    grad = torch.zeros(N, k * k * C_, device="cuda")
    ws = torch.zeros(16, device="cuda")
    with pytest.raises(_lib.MemhipError, match="workspace 64 <"):
        ops.conv_wgrad(small, big, grad, B, Hs, Ws, C_, N, k, s, pad, workspace=ws)
    with pytest.raises(_lib.MemhipError, match="need a 16-byte aligned workspace"):
        ops.conv_wgrad(small, big, grad, B, Hs, Ws, C_, N, k, s, pad, workspace=None)


# ---------------------------------------------------------------- relu_bwd_colsum
@pytest.mark.parametrize("B,H,W,C_,padded,masked", [(3, 5, 7, 72, True, True), (2, 12, 20, 384, True, True), (3, 5, 7, 8, False, True),
                                                    (2, 3, 5, 2056, False, True), (3, 5, 7, 64, True, False)])
def test_relu_bwd_colsum(B, H, W, C_, padded, masked):
    """The masked g equals torch's bit for bit, the ring is untouched (g's holds 3, y's +1: a masked ring would still pass the
    mask), the column sums are within R * 2^-23 * sum |g| of float64, and a second call gives the same bits."""
    from mem_amd import ops
    R = B * H * W
    gen = torch.Generator().manual_seed(C_ + H)
    gi = torch.randn(B, H, W, C_, generator=gen).bfloat16()
    yi = torch.relu(torch.randn(B, H, W, C_, generator=gen)).bfloat16()
    if padded:
        g = torch.full((B, H + 2, W + 2, C_), 3.0, dtype=torch.bfloat16)
        y = torch.ones((B, H + 2, W + 2, C_), dtype=torch.bfloat16)
        g[:, 1:-1, 1:-1], y[:, 1:-1, 1:-1] = gi, yi
    else:
        g, y = gi.reshape(R, C_).clone(), yi.reshape(R, C_).clone()
    want_g = g.clone()
    inner = torch.where(yi > 0, gi, torch.zeros_like(gi)) if masked else gi
    if padded:
        want_g[:, 1:-1, 1:-1] = inner
    else:
        want_g = inner.reshape(R, C_)
    want_sum = inner.double().reshape(R, C_).sum(0)
    bound = R * 2.0 ** -23 * inner.double().abs().reshape(R, C_).sum(0)
    nbytes = ops.relu_bwd_colsum_workspace(B, H, W, C_)
    outs = []
    for _ in range(2):
        gd = g.cuda()
        ws = torch.full((nbytes // 4,), NAN, device="cuda")
        colsum = torch.full((C_,), NAN, device="cuda")
        ops.relu_bwd_colsum(gd, y.cuda() if masked else None, B, H, W, C_, padded=padded, colsum=colsum, workspace=ws)
        assert torch.equal(gd.cpu(), want_g)
        assert bool(((colsum.cpu().double() - want_sum).abs() <= bound).all())
        outs.append(colsum.clone())
    assert torch.equal(outs[0], outs[1])
    # accumulate onto a bias gradient; and the mask alone (no sums, no workspace)
    pre = torch.randn(C_, generator=gen)
    colsum = pre.clone().cuda()
    ops.relu_bwd_colsum(g.cuda(), y.cuda() if masked else None, B, H, W, C_, padded=padded, colsum=colsum, accumulate=True,
                        workspace=torch.full((nbytes // 4,), NAN, device="cuda"))
    assert bool(((colsum.cpu().double() - pre.double() - want_sum).abs() <= bound + 2.0 ** -23 * (pre.abs() + want_sum.abs())).all())
    if masked:
        gd = g.cuda()
        ops.relu_bwd_colsum(gd, y.cuda(), B, H, W, C_, padded=padded)
        assert torch.equal(gd.cpu(), want_g)


# ---------------------------------------------------------------- the data gradients: forward kernels, re-read weights
def _pad_nhwc(t):
    """[B, C, H, W] -> bf16 padded NHWC on the GPU, zero ring."""
    B, C_, H, W = t.shape
    out = torch.zeros(B, H + 2, W + 2, C_, dtype=torch.bfloat16, device="cuda")
    out[:, 1:-1, 1:-1] = t.permute(0, 2, 3, 1).to(torch.bfloat16)
    return out


def _autograd_dx(fwd, x_shape, g):
    x = torch.zeros(x_shape, requires_grad=True)
    fwd(x).backward(g)
    return x.grad


def _close(got_nchw, ref):
    torch.testing.assert_close(got_nchw.float().cpu(), ref.bfloat16().float(), rtol=2e-2, atol=2e-2)


def test_dgrad_conv4s2_is_convt2d():
    from mem_amd import ops
    from mem_amd.vae_model import pack_dgrad_weight
    B, ci, co, H, W = 2, 72, 64, 10, 14                     # layer Conv2d(ci, co, 4, 2, 1) on H x W; g on H/2 x W/2
    gen = torch.Generator().manual_seed(1)
    w = (torch.randn(co, ci, 4, 4, generator=gen) * (4.0 / (4 * co)) ** 0.5).bfloat16().float()
    g = torch.randn(B, co, H // 2, W // 2, generator=gen).bfloat16().float()
    ref = _autograd_dx(lambda x: F.conv2d(x, w, stride=2, padding=1), (B, ci, H, W), g)
    out = torch.zeros(B, H + 2, W + 2, ci, dtype=torch.bfloat16, device="cuda")
    ops.convt2d_nhwc(_pad_nhwc(g), pack_dgrad_weight("conv4s2", w).bfloat16().cuda(), None, out, B, H // 2, W // 2, co, ci)
    _close(out[:, 1:-1, 1:-1].permute(0, 3, 1, 2), ref)


def test_dgrad_convt_is_conv2d_4s2():
    from mem_amd import ops
    from mem_amd.vae_model import pack_dgrad_weight
    B, ci, co, H, W = 2, 72, 64, 5, 7                       # layer ConvTranspose2d(ci, co, 4, 2, 1) on H x W; g on 2H x 2W
    gen = torch.Generator().manual_seed(2)
    w = (torch.randn(ci, co, 4, 4, generator=gen) * (1.0 / (16 * co)) ** 0.5).bfloat16().float()
    g = torch.randn(B, co, 2 * H, 2 * W, generator=gen).bfloat16().float()
    ref = _autograd_dx(lambda x: F.conv_transpose2d(x, w, stride=2, padding=1), (B, ci, H, W), g)
    out = torch.zeros(B, H + 2, W + 2, ci, dtype=torch.bfloat16, device="cuda")
    ops.conv2d_nhwc(_pad_nhwc(g), pack_dgrad_weight("convt", w).bfloat16().cuda(), None, out, B, 2 * H, 2 * W, co, ci, 4, 2, 1)
    _close(out[:, 1:-1, 1:-1].permute(0, 3, 1, 2), ref)


@pytest.mark.parametrize("kind,k,pad", [("conv3", 3, 1), ("conv1", 1, 0)])
def test_dgrad_conv3_conv1_with_the_resblock_add(kind, k, pad):
    """Conv2d(3, 1, 1) and Conv2d(1) between padded buffers; with add= the ResBlock's dX = dgrad(g1) + g."""
    from mem_amd import ops
    from mem_amd.vae_model import pack_dgrad_weight
    B, ci, co, H, W = 2, 72, 128, 5, 7
    gen = torch.Generator().manual_seed(3 + k)
    w = (torch.randn(co, ci, k, k, generator=gen) * (1.0 / (k * k * co)) ** 0.5).bfloat16().float()
    g = torch.randn(B, co, H, W, generator=gen).bfloat16().float()
    skip = torch.randn(B, ci, H, W, generator=gen).bfloat16().float()
    ref = _autograd_dx(lambda x: F.conv2d(x, w, padding=pad), (B, ci, H, W), g)
    wp = pack_dgrad_weight(kind, w).bfloat16().cuda()
    out = torch.zeros(B, H + 2, W + 2, ci, dtype=torch.bfloat16, device="cuda")
    ops.conv2d_nhwc(_pad_nhwc(g), wp, None, out, B, H, W, co, ci, k, 1, pad)
    _close(out[:, 1:-1, 1:-1].permute(0, 3, 1, 2), ref)
    ops.conv2d_nhwc(_pad_nhwc(g), wp, None, out, B, H, W, co, ci, k, 1, pad, add=_pad_nhwc(skip))
    _close(out[:, 1:-1, 1:-1].permute(0, 3, 1, 2), ref + skip)


@pytest.mark.parametrize("co,copad", [(512, 512), (3, 64)])
def test_dgrad_heads_are_nt_gemms(co, copad):
    """The two 1x1 heads with a dense g [M, co]: dX = g @ W through memhip_gemm_bf16_nt with W^T [ci, co]; the reconstruction
    head's 3 (8) channels are zero-padded to 64 for the GEMM's K."""
    from mem_amd import ops
    from mem_amd.vae_model import pack_dgrad_weight
    B, ci, H, W = 3, 64, 5, 7
    M = B * H * W
    gen = torch.Generator().manual_seed(co)
    w = (torch.randn(co, ci, 1, 1, generator=gen) * (1.0 / co) ** 0.5).bfloat16().float()
    g = torch.randn(B, co, H, W, generator=gen).bfloat16().float()
    ref = _autograd_dx(lambda x: F.conv2d(x, w), (B, ci, H, W), g)
    wt = pack_dgrad_weight("conv1", w, cin_pad=copad).bfloat16().cuda()               # [ci, copad]
    gd = F.pad(g.permute(0, 2, 3, 1).reshape(M, co), (0, copad - co)).bfloat16().contiguous().cuda()
    dense = torch.empty(M, ci, dtype=torch.bfloat16, device="cuda")
    ops.gemm_nt(gd, wt, M, ci, copad, ops.EPI_BIAS_BF16, out0=dense)
    out = torch.zeros(B, H + 2, W + 2, ci, dtype=torch.bfloat16, device="cuda")
    out[:, 1:-1, 1:-1] = dense.view(B, H, W, ci)                                       # copied into the interior
    _close(out[:, 1:-1, 1:-1].permute(0, 3, 1, 2), ref)
