"""-m "not gpu": the host side of the fused feature-pyramid necks -- the index algebra of the interleaved / nested orders
(float64, through the packing helpers the product uses), the entry points declared, exported and bound, their argument
checks in front of any launch, and EvBEiT(necks=...) with the torch modules' state-dict keys in both modes."""
import os

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(img_size=(32, 48), patch_size=(16, 16), in_chans=3, embed_dim=64, depth=6, num_heads=1, mlp_ratio=4,
             drop_path_rate=0.1, init_values=0.1, use_abs_pos_emb=False, use_rel_pos_bias=True)
NAMES = ("memhip_neck_maps_to_rows", "memhip_neck_rows_to_maps", "memhip_neck_colstats", "memhip_neck_bn_gelu_fwd",
         "memhip_neck_bn_gelu_bwd_sums", "memhip_neck_bn_gelu_bwd_apply")


def _conv(g, D):
    return (torch.randn((D, D, 2, 2), generator=g, dtype=torch.float64), torch.randn(D, generator=g, dtype=torch.float64))


@pytest.mark.parametrize("B,D,Hp,Wp", [(2, 3, 2, 3), (1, 5, 3, 2), (3, 4, 1, 5)])
def test_transposed_convolution_is_rows_times_weight_matrix(B, D, Hp, Wp):
    """One level: conv_transpose2d(x, W, b, stride 2) == rows_to_map(map_to_rows(x, 0) @ weight_matrix(W) + bias_operand(b), 1),
    and map_to_rows(., 1) of it gives the product back.  Two levels: the second product runs on the DE-INTERLEAVED rows
    Z[4r + q, co] = Y[r, 4 co + q] of the first, and rows_to_map(., 2) places the nested order.  float64, exact to rounding of
    the differently ordered sums."""
    from mem_amd import necks as N
    g = torch.Generator().manual_seed(B * 100 + D * 10 + Hp)
    x = torch.randn((B, D, Hp, Wp), generator=g, dtype=torch.float64)
    (W1, b1), (W2, b2) = _conv(g, D), _conv(g, D)
    R = B * Hp * Wp
    X = N.map_to_rows(x, 0)
    assert tuple(X.shape) == (R, D) and torch.equal(X[Wp + 1 if Hp > 1 else 1], x[0, :, 1 if Hp > 1 else 0, 1])
    Y1 = X @ N.weight_matrix(W1) + N.bias_operand(b1)
    want1 = F.conv_transpose2d(x, W1, b1, stride=2)
    got1 = N.rows_to_map(Y1, B, D, Hp, Wp, 1)
    assert tuple(got1.shape) == (B, D, 2 * Hp, 2 * Wp)
    assert torch.allclose(got1, want1, rtol=0, atol=1e-12)
    assert torch.equal(N.map_to_rows(got1, 1), Y1)                                  # the two helpers invert each other
    Z1 = Y1.reshape(R, D, 4).transpose(1, 2).reshape(4 * R, D)                      # Z[4r + q, co] = Y[r, 4 co + q]
    assert torch.equal(Z1, N.map_to_rows(got1, 0).reshape(B, Hp, 2, Wp, 2, D).permute(0, 1, 3, 2, 4, 5).reshape(4 * R, D))
    Y2 = Z1 @ N.weight_matrix(W2) + N.bias_operand(b2)
    want2 = F.conv_transpose2d(want1, W2, b2, stride=2)
    got2 = N.rows_to_map(Y2, B, D, Hp, Wp, 2)
    assert tuple(got2.shape) == (B, D, 4 * Hp, 4 * Wp)
    assert torch.allclose(got2, want2, rtol=0, atol=1e-11)
    assert torch.equal(N.map_to_rows(got2, 2), Y2)
    # the documented nested order, spelled out for one element: row 4 r0 + (2 ia + ja), column 4 co + (2 ib + jb)
    b, y, xx, ia, ja, ib, jb, co = B - 1, Hp - 1, Wp - 1, 1, 0, 0, 1, D - 1
    r0 = (b * Hp + y) * Wp + xx
    assert Y2[4 * r0 + 2 * ia + ja, 4 * co + 2 * ib + jb] == got2[b, co, 4 * y + 2 * ia + ib, 4 * xx + 2 * ja + jb]


def test_gradients_in_the_kept_column_order():
    """dX = dY W^T with the [D, 4D] matrix as it lies, dW = X^T dY in W.grad's own layout, dbias = fold4(colsum dY): float64
    autograd of conv_transpose2d agrees."""
    from mem_amd import necks as N
    g = torch.Generator().manual_seed(7)
    B, D, Hp, Wp = 2, 3, 2, 3
    x = torch.randn((B, D, Hp, Wp), generator=g, dtype=torch.float64, requires_grad=True)
    W, b = _conv(g, D)
    W.requires_grad_(True), b.requires_grad_(True)
    dout = torch.randn((B, D, 2 * Hp, 2 * Wp), generator=g, dtype=torch.float64)
    F.conv_transpose2d(x, W, b, stride=2).backward(dout)
    dY = N.map_to_rows(dout, 1)
    X = N.map_to_rows(x.detach(), 0)
    assert torch.allclose(N.rows_to_map(dY @ N.weight_matrix(W.detach()).t(), B, D, Hp, Wp, 0), x.grad, rtol=0, atol=1e-12)
    assert torch.allclose((X.t() @ dY).reshape(D, D, 2, 2), W.grad, rtol=0, atol=1e-12)
    assert torch.allclose(N.fold4(dY.sum(0)), b.grad, rtol=0, atol=1e-12)


def _lib():
    from mem_amd import _lib, ops  # noqa: F401  (ops declares the signatures)
    return _lib.lib


def test_neck_symbols_are_declared_exported_and_bound():
    lib = _lib()
    from mem_amd import ops
    header = open(os.path.join(ROOT, "include", "memhip.h")).read()
    for name in NAMES:
        assert f"int {name}(" in header, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
        assert callable(getattr(ops, name[len("memhip_"):])), name
    assert "size_t memhip_neck_sums_workspace(" in header
    assert lib.memhip_neck_sums_workspace(768) == ops.NECK_GROUPS * 2 * 768 * 4
    assert f"#define MEMHIP_NECK_GROUPS {ops.NECK_GROUPS}\n" in header


def _bad(rc, lib, word):
    assert rc == -1, rc
    assert word.encode() in lib.memhip_last_error(), lib.memhip_last_error()


def test_neck_entries_validate_before_any_launch():
    """Bad shapes, levels, null and misaligned pointers and a short workspace return MEMHIP_EINVAL with a message; nothing is
    launched (no GPU here)."""
    import ctypes as C
    import numpy as np
    lib = _lib()
    buf = np.zeros(256, dtype=np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    p, odd = C.c_void_p(base), C.c_void_p(base + 4)
    for fn, tag in ((lib.memhip_neck_maps_to_rows, "neck_maps_to_rows"), (lib.memhip_neck_rows_to_maps, "neck_rows_to_maps")):
        # (src, B, D, Hp, Wp, level, dst, stream)
        _bad(fn(p, 1, 96, 2, 2, 0, p, None), lib, tag + ": bad shape")             # D % 64 != 0
        _bad(fn(p, 0, 64, 2, 2, 0, p, None), lib, tag + ": bad shape")
        _bad(fn(p, 1, 64, 2, 0, 1, p, None), lib, tag + ": bad shape")
        _bad(fn(p, 1, 64, 2, 2, 3, p, None), lib, tag + ": bad level")
        _bad(fn(p, 1, 64, 2, 2, -1, p, None), lib, tag + ": bad level")
        _bad(fn(None, 1, 64, 2, 2, 0, p, None), lib, "null pointer")
        _bad(fn(p, 1, 64, 2, 2, 0, None, None), lib, "null pointer")
    _bad(lib.memhip_neck_maps_to_rows(p, 1, 64, 2, 2, 0, odd, None), lib, "rows is not 16-byte aligned")
    _bad(lib.memhip_neck_maps_to_rows(odd, 1, 64, 2, 2, 2, p, None), lib, "map is not aligned")
    _bad(lib.memhip_neck_rows_to_maps(odd, 1, 64, 2, 2, 0, p, None), lib, "rows is not 16-byte aligned")
    _bad(lib.memhip_neck_rows_to_maps(p, 1, 64, 2, 2, 1, odd, None), lib, "map is not aligned")
    ws = lib.memhip_neck_sums_workspace(64)
    # memhip_neck_colstats(y, R, D, shift, ws, ws_bytes, out, stream)
    _bad(lib.memhip_neck_colstats(p, 0, 64, p, p, ws, p, None), lib, "bad shape")
    _bad(lib.memhip_neck_colstats(p, 4, 100, p, p, ws, p, None), lib, "bad shape")
    _bad(lib.memhip_neck_colstats(p, 4, 64, None, p, ws, p, None), lib, "null pointer")
    _bad(lib.memhip_neck_colstats(p, 4, 64, p, p, ws - 4, p, None), lib, "workspace")
    _bad(lib.memhip_neck_colstats(odd, 4, 64, p, p, ws, p, None), lib, "16-byte aligned")
    # memhip_neck_bn_gelu_fwd(y, R, D, mean, rstd, gamma, beta, z, stream)
    _bad(lib.memhip_neck_bn_gelu_fwd(p, 4, 32, p, p, p, p, p, None), lib, "bad shape")
    _bad(lib.memhip_neck_bn_gelu_fwd(p, 4, 64, p, None, p, p, p, None), lib, "null pointer")
    _bad(lib.memhip_neck_bn_gelu_fwd(p, 4, 64, p, p, p, p, None, None), lib, "null pointer")
    _bad(lib.memhip_neck_bn_gelu_fwd(p, 4, 64, p, p, p, p, odd, None), lib, "16-byte aligned")
    # memhip_neck_bn_gelu_bwd_sums(da, y, R, D, mean, rstd, gamma, beta, ws, ws_bytes, out, stream)
    _bad(lib.memhip_neck_bn_gelu_bwd_sums(p, p, -1, 64, p, p, p, p, p, ws, p, None), lib, "bad shape")
    _bad(lib.memhip_neck_bn_gelu_bwd_sums(None, p, 4, 64, p, p, p, p, p, ws, p, None), lib, "null pointer")
    _bad(lib.memhip_neck_bn_gelu_bwd_sums(p, p, 4, 64, p, p, p, p, p, 16, p, None), lib, "workspace")
    # memhip_neck_bn_gelu_bwd_apply(da, y, R, D, mean, rstd, gamma, beta, sums, inv_n, dy, stream)
    _bad(lib.memhip_neck_bn_gelu_bwd_apply(p, p, 4, 96, p, p, p, p, p, 1.0, p, None), lib, "bad shape")
    _bad(lib.memhip_neck_bn_gelu_bwd_apply(p, p, 4, 64, p, p, p, p, None, 1.0, p, None), lib, "null pointer")
    _bad(lib.memhip_neck_bn_gelu_bwd_apply(p, p, 4, 64, p, p, p, p, p, 0.0, p, None), lib, "inv_n")
    _bad(lib.memhip_neck_bn_gelu_bwd_apply(p, p, 4, 64, p, p, p, p, p, 1.0, odd, None), lib, "16-byte aligned")
    assert float(np.abs(buf).max()) == 0.0


def test_evbeit_necks_argument_and_state_dict_keys():
    from mem_amd.semseg_backbone import EvBEiT
    a = EvBEiT(out_indices=(1, 2, 3, 5), **SMALL)
    b = EvBEiT(out_indices=(1, 2, 3, 5), necks="torch", **SMALL)
    c = EvBEiT(out_indices=(1, 2, 3, 5), necks="fused", **SMALL)
    assert a.necks == "torch" and b.necks == "torch" and c.necks == "fused"
    keys = list(a.state_dict().keys())
    assert list(b.state_dict().keys()) == keys and list(c.state_dict().keys()) == keys
    assert all(a.state_dict()[k].shape == c.state_dict()[k].shape and a.state_dict()[k].dtype == c.state_dict()[k].dtype for k in keys)
    assert c._ctor_kwargs["necks"] == "fused"                                    # an EMA twin is built in the same mode
    c.load_state_dict(a.state_dict())                                             # a checkpoint moves between the modes
    a.load_state_dict(c.state_dict())
    assert a._engine is None and c._engine is None and c._fused_necks is None   # nothing touched the GPU
    with pytest.raises(ValueError) as e:
        EvBEiT(necks="triton", **SMALL)
    assert "necks" in str(e.value) and "triton" in str(e.value)
