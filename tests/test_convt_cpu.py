"""-m "not gpu": the host side of the tokenizer's decoder (csrc/convt.hip, conv_plan.cpp, mem_amd/vae_model.py).

The weight layout of memhip_convt2d_nhwc is a contract between pack_convt_weight and the kernel: it is restated here in float64
from the packed tensor alone and compared with F.conv_transpose2d.  memhip_convt_plan's geometry, and every rejection rule of
the three new entry points, are exercised through ctypes with dummy addresses -- nothing reaches a launch."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

SHAPES = [(2, 64, 72, 3, 5), (1, 128, 8, 4, 3)]           # (B, Cin, Cout, H, W): non-square, no multiple of any tile
P = 0x1000                                                  # a dummy, 16-byte aligned, non-NULL address


def test_symbols_exported_and_abi_unchanged():
    from mem_amd import _lib
    for name in ("memhip_convt2d_nhwc", "memhip_convt_plan", "memhip_kl_uniform_rows"):
        assert hasattr(_lib.lib, name), name
    assert _lib.lib.memhip_abi_version() == 10


def phase_sum(x, packed, bias):
    """The four-phase sum of include/memhip.h, from the PACKED weight only.  x [B, Cin, H, W], packed [4, Cout, 4 Cin]."""
    B, Cin, H, W = x.shape
    Cout = packed.shape[1]
    xp = F.pad(x.permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1))                 # [B, H+2, W+2, Cin], zero border
    out = torch.zeros(B, 2 * H, 2 * W, Cout, dtype=x.dtype)
    for py in (0, 1):
        for px in (0, 1):
            wk = packed[2 * py + px].view(Cout, 2, 2, Cin)
            acc = bias.view(1, 1, 1, Cout).expand(B, H, W, Cout).clone()
            for dy in (0, 1):
                for dx in (0, 1):
                    win = xp[:, py + dy: py + dy + H, px + dx: px + dx + W]      # in_pad[b, y+py+dy, x+px+dx, :]
                    acc = acc + torch.einsum("byxc,oc->byxo", win, wk[:, dy, dx])
            out[:, py::2, px::2] = acc
    return out.permute(0, 3, 1, 2)


@pytest.mark.parametrize("B,Cin,Cout,H,W", SHAPES)
def test_packing_contract(B, Cin, Cout, H, W):
    from mem_amd import ops
    g = torch.Generator().manual_seed(Cin + Cout)
    x = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Cin, Cout, 4, 4, generator=g, dtype=torch.float64)
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    packed = ops.pack_convt_weight(w)
    assert packed.shape == (4, Cout, 4 * Cin) and packed.dtype == torch.float64 and packed.is_contiguous()
    want = F.conv_transpose2d(x, w, b, stride=2, padding=1)
    got = phase_sum(x, packed, b)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= 1e-12
    # zero-padded channel counts (what HipTokenizer.decode does for a 32-dim codebook): the extra rows / columns are zeros
    pp = ops.pack_convt_weight(w, cin_pad=Cin + 64, cout_pad=Cout + 8)
    assert pp.shape == (4, Cout + 8, 4 * (Cin + 64))
    v = pp.view(4, Cout + 8, 4, Cin + 64)
    assert torch.equal(v[:, :Cout, :, :Cin].reshape(4, Cout, 4 * Cin), packed)
    assert v[:, Cout:].abs().max() == 0 and v[:, :, :, Cin:].abs().max() == 0


@pytest.mark.parametrize("B,Cin,Cout,H,W", SHAPES + [(2, 384, 384, 112, 112)])
def test_convt_plan_geometry(B, Cin, Cout, H, W):
    from mem_amd import ops
    p = ops.convt_plan(B, H, W, Cin, Cout, device_cus=256)
    M = B * H * W
    assert (p.Hp, p.Wp, p.Ho, p.Wo, p.K, p.off, p.M, p.count) == (H + 2, W + 2, 2 * H, 2 * W, 4 * Cin, 0, M, 1)
    tiles = -(-M // 128) * -(-Cout // 128)
    (name, grid, block, lds, lo, hi), = p.launches
    assert name == "convt_gemm_kernel" and p.l[0].kernel == len(ops.CONV_KERNELS) - 1      # the new, last enumerator
    assert grid == 4 * tiles and block == 256 and 0 < lds <= 160 * 1024
    assert (lo, hi) == (0, 1 << 30)
    empty = ops.convt_plan(0, H, W, Cin, Cout, device_cus=256)
    assert empty.M == 0 and empty.count == 0 and empty.launches == []


def _err():
    from mem_amd import _lib
    return _lib.lib.memhip_last_error().decode()


def test_convt_validation_and_the_plan_query_agree():
    from mem_amd import _lib, ops
    lib = _lib.lib

    def call(B=2, H=3, W=5, Cin=64, Cout=72, x=P, w=P, out=P):
        rc = lib.memhip_convt2d_nhwc(x, w, None, out, B, H, W, Cin, Cout, 0, None)
        return rc, _err()

    def query(B=2, H=3, W=5, Cin=64, Cout=72):
        rc = lib.memhip_convt_plan(B, H, W, Cin, Cout, 256, C.byref(ops.ConvPlan()))
        return rc, _err()

    for bad, message in ((dict(Cin=96), "convt2d: C_in must be a multiple of 64"),
                         (dict(Cin=32), "convt2d: C_in must be a multiple of 64"),
                         (dict(Cout=12), "convt2d: C_out must be a multiple of 8"),
                         (dict(H=0), "convt2d: bad shape"), (dict(W=0), "convt2d: bad shape"),
                         (dict(H=-2), "convt2d: bad shape"), (dict(W=-1), "convt2d: bad shape"),
                         (dict(B=-1), "convt2d: bad shape"), (dict(Cin=0), "convt2d: bad shape"),
                         (dict(B=1 << 16, H=128, W=128), "convt2d: too many output pixels")):
        rc, err = call(**bad)
        assert rc == -1 and message in err, (bad, rc, err)
        assert query(**bad) == (rc, err), bad
    # the call alone needs its pointers; the query asks about a call it does not make
    for field in ("x", "w", "out"):
        rc, err = call(**{field: None})
        assert rc == -1 and "convt2d: null pointer" in err
    assert query()[0] == 0
    rc = lib.memhip_convt_plan(2, 3, 5, 64, 72, 256, None)
    assert rc == -1 and "convt_plan: null pointer" in _err()
    # an empty batch: nothing to do, nothing read
    assert call(B=0, x=None, w=None, out=None)[0] == 0 and query(B=0)[0] == 0


def test_kl_uniform_rows_validation():
    from mem_amd import _lib
    lib = _lib.lib
    BF16, F32 = 0, 1

    def call(mode=F32, ld=512, M=4, N=512, logits=P, out=P):
        return lib.memhip_kl_uniform_rows(logits, mode, ld, M, N, out, None), _err()

    for mode in (2, 3, -1):                                 # fp16x2 activations have fp32 logits: not a logit type
        rc, err = call(mode=mode)
        assert rc == -1 and "kl_uniform_rows: the logits are bf16 or fp32, mode %d" % mode in err
    for bad in (dict(N=510, ld=512), dict(ld=514), dict(N=0), dict(N=512, ld=256)):
        rc, err = call(mode=F32, **bad)
        assert rc == -1 and "kl_uniform_rows: N and ld must be multiples of 4" in err, bad
    for bad in (dict(N=508, ld=512), dict(ld=516), dict(N=0)):          # multiples of 4, not of 8
        rc, err = call(mode=BF16, **bad)
        assert rc == -1 and "kl_uniform_rows: N and ld must be multiples of 8" in err, bad
    for bad in (dict(logits=None), dict(out=None)):
        rc, err = call(**bad)
        assert rc == -1 and "kl_uniform_rows: null pointer" in err
    assert call(M=0, logits=None, out=None)[0] == 0


def test_discrete_vae_losses_and_forward_still_refuses():
    from mem_amd.vae_model import DiscreteVAE
    cfg = dict(input_H=16, input_W=16, num_tokens=16, codebook_dim=8, num_layers=2, hidden_dim=8)
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(2, 3, 16, 16, generator=g), torch.randn(2, 3, 16, 16, generator=g)

    def cosine(target, rec):                                # vae_model.py:116-119
        target = target / (target.norm(dim=-1, keepdim=True) + 1e-9)
        rec = rec / (rec.norm(dim=-1, keepdim=True) + 1e-9)
        return (1 - (target * rec).sum(-1)).mean()
    for loss, want in (("mse", F.mse_loss(a, b)), ("smooth_l1", F.smooth_l1_loss(a, b)), ("cosine", cosine(a, b))):
        m = DiscreteVAE(loss=loss, temperature=0.7, straight_through=True, kl_div_loss_weight=0.25, **cfg)
        assert (m.loss, m.temperature, m.straight_through, m.kl_div_loss_weight) == (loss, 0.7, True, 0.25)
        assert torch.equal(m.loss_fn(a, b), want), loss
    m = DiscreteVAE(**cfg)                                  # the defaults are the reference's
    assert (m.loss, m.temperature, m.straight_through, m.kl_div_loss_weight) == ("mse", 0.9, False, 0.0)
    with pytest.raises(KeyError):
        DiscreteVAE(loss="l3", **cfg)
    with pytest.raises(NotImplementedError):
        m(a)
    assert m(a, return_logits=True).shape == (2, 16, 4, 4)
    # loss_fn is no parameter and no buffer: reference checkpoints still load by key
    assert not any("loss" in k for k in m.state_dict())
