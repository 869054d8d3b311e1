"""-m "not gpu": the FCN decode head without a device -- the validation and the plan of the new entry points (host arithmetic),
FCNHead(impl="torch") in float64 against a hand-written expression of the same layers, the running statistics against
nn.BatchNorm2d, the state-dict keys against mmseg's, and the refused arguments.

``oracle_head`` is the float64 oracle of tests/test_seg_head_gpu.py too."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

EINVAL = -1
FAKE = 0x10000            # a non-null, 16-byte aligned address: validation never dereferences a pointer
# (B, Cin, C, K, h, w): the cases of the GPU tests
CASES = {"S1": (2, 64, 64, 3, 5, 7), "S2": (3, 128, 128, 19, 6, 10), "S3": (1, 768, 256, 11, 4, 6),
         "S1K2": (2, 64, 64, 2, 5, 7), "S1K32": (2, 64, 64, 32, 5, 7),
         "MAX": (1, 64, 512, 32, 3, 5),       # the largest head the kernels accept: the classifier weight fills the forward's 64 KiB of LDS
         "BIG": (2, 64, 64, 3, 96, 97)}       # 18 624 pixels: more tiles than workgroups in the forward (512), the sums and the statistics (128)
MMSEG_KEYS = {"convs.0.conv.weight": ("channels", "in_channels", 3, 3), "convs.0.bn.weight": ("channels",),
              "convs.0.bn.bias": ("channels",), "convs.0.bn.running_mean": ("channels",), "convs.0.bn.running_var": ("channels",),
              "convs.0.bn.num_batches_tracked": (), "conv_seg.weight": ("num_classes", "channels", 1, 1),
              "conv_seg.bias": ("num_classes",)}


# ---------------------------------------------------------------------------------------------- the float64 oracle
def oracle_head(x, w, gamma, beta, wcls, bcls, keep=None, p=0.0, eps=1e-5, running=None):
    """conv 3x3 (zero padding 1, no bias) -> batch norm (batch statistics with the biased variance, or ``running`` = (mean, var))
    -> relu -> channel mask ``keep`` [B, C] (0 / 1) / (1 - p) -> 1x1 classifier, written out by hand; any dtype, differentiable.
    x [B, Cin, h, w], w [C, Cin, 3, 3], wcls [K, C]."""
    B, Cin, h, wd = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    y = sum(torch.einsum("bihw,oi->bohw", xp[:, :, ky:ky + h, kx:kx + wd], w[:, :, ky, kx]) for ky in range(3) for kx in range(3))
    if running is None:
        mean = y.mean(dim=(0, 2, 3))
        var = ((y - mean[None, :, None, None]) ** 2).mean(dim=(0, 2, 3))
    else:
        mean, var = running
    xhat = (y - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + eps)
    z = torch.clamp(gamma[None, :, None, None] * xhat + beta[None, :, None, None], min=0.0)
    if keep is not None:
        z = z * (keep.to(z.dtype) / (1.0 - p))[:, :, None, None]
    return torch.einsum("bchw,kc->bkhw", z, wcls) + bcls[None, :, None, None]


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ---------------------------------------------------------------------------------------------- validation and plan
def _args(ops, B=2, C=64, K=3, h=5, w=7, **kw):
    fields = dict(y=FAKE, mean=FAKE, rstd=FAKE, gamma=FAKE, beta=FAKE, wcls=FAKE, bias=FAKE, logits=FAKE, ld=K, dlogit=FAKE,
                  db=K * h * w, dk=1, dy=w * K, dx=K, sums=FAKE, dwcls=FAKE, dbias=FAKE, workspace=FAKE, workspace_bytes=1 << 30,
                  tot=FAKE, inv_n=0.5, dy_out=FAKE)
    fields.update(kw)
    return ops.bnhead_args(B, C, K, h, w, **fields)


BAD = [("C % 64", dict(C=96), b"C=96"), ("K = 1", dict(K=1), b"K=1"), ("K = 33", dict(K=33), b"K=33"), ("C = 576", dict(C=576), b"C=576"),
       ("ld < K", dict(K=3, ld=2), b"ld=2")]


@pytest.mark.parametrize("name,kw,word", BAD, ids=[b[0] for b in BAD])
def test_bad_shapes_are_rejected_before_any_launch(name, kw, word):
    from mem_amd import ops
    from mem_amd._lib import lib
    a = _args(ops, **kw)
    plan = ops.BnHeadPlan()
    rc_plan = lib.memhip_bnhead_plan(ctypes.byref(a), ctypes.byref(plan))
    msg_plan = lib.memhip_last_error()
    calls = [lib.memhip_bnhead_fwd] if name == "ld < K" else [lib.memhip_bnhead_fwd, lib.memhip_bnhead_bwd_sums, lib.memhip_bnhead_bwd_apply]
    for call in calls:
        rc = call(ctypes.byref(a), None)
        msg = lib.memhip_last_error()
        print(name, rc, rc_plan, msg)
        assert rc == EINVAL == rc_plan and word in msg and msg == msg_plan


@pytest.mark.parametrize("call,field", [("memhip_bnhead_fwd", "y"), ("memhip_bnhead_fwd", "logits"), ("memhip_bnhead_fwd", "wcls"),
                                        ("memhip_bnhead_bwd_sums", "dlogit"), ("memhip_bnhead_bwd_sums", "workspace"),
                                        ("memhip_bnhead_bwd_sums", "dwcls"), ("memhip_bnhead_bwd_apply", "dy_out"),
                                        ("memhip_bnhead_bwd_apply", "rstd")])
def test_a_null_required_pointer_is_rejected(call, field):
    from mem_amd import ops
    from mem_amd._lib import lib
    rc = getattr(lib, call)(ctypes.byref(_args(ops, **{field: None})), None)
    print(call, field, rc, lib.memhip_last_error())
    assert rc == EINVAL and b"null" in lib.memhip_last_error()
    assert lib.memhip_bnhead_fwd(None, None) == EINVAL


def test_misaligned_pointers_small_workspace_and_bad_inv_n():
    from mem_amd import ops
    from mem_amd._lib import lib
    assert lib.memhip_bnhead_fwd(ctypes.byref(_args(ops, y=FAKE + 2)), None) == EINVAL and b"aligned" in lib.memhip_last_error()
    assert lib.memhip_bnhead_bwd_sums(ctypes.byref(_args(ops, workspace_bytes=16)), None) == -2       # MEMHIP_EWORKSPACE
    plan = ops.BnHeadPlan()
    assert lib.memhip_bnhead_plan(ctypes.byref(_args(ops, workspace_bytes=16)), ctypes.byref(plan)) == -2
    assert lib.memhip_bnhead_bwd_apply(ctypes.byref(_args(ops, inv_n=0.0)), None) == EINVAL and b"inv_n" in lib.memhip_last_error()


def test_movers_and_statistics_validate():
    from mem_amd._lib import lib
    for fn in (lib.memhip_map_to_nhwc_pad, lib.memhip_nhwc_pad_to_map):
        assert fn(FAKE, 2, 96, 5, 7, FAKE, None) == EINVAL and b"multiple of 64" in lib.memhip_last_error()
        assert fn(FAKE, 2, 64, 0, 7, FAKE, None) == EINVAL
        assert fn(None, 2, 64, 5, 7, FAKE, None) == EINVAL and b"null" in lib.memhip_last_error()
        assert fn(None, 0, 64, 5, 7, None, None) == 0                                                 # B == 0: nothing to do
    assert lib.memhip_map_to_nhwc_pad(FAKE, 2, 64, 5, 7, FAKE + 8, None) == EINVAL and b"aligned" in lib.memhip_last_error()
    st = lib.memhip_bn_stats_nhwc
    assert st(FAKE, 1, 2, 5, 7, 96, None, FAKE, 1 << 20, FAKE, None) == EINVAL
    assert st(FAKE, 2, 2, 5, 7, 64, None, FAKE, 1 << 20, FAKE, None) == EINVAL and b"padded" in lib.memhip_last_error()
    assert st(None, 1, 2, 5, 7, 64, None, FAKE, 1 << 20, FAKE, None) == EINVAL and b"null" in lib.memhip_last_error()
    assert st(FAKE, 1, 2, 5, 7, 64, None, FAKE, 16, FAKE, None) == EINVAL and b"workspace" in lib.memhip_last_error()
    assert st(None, 1, 0, 5, 7, 64, None, None, 0, None, None) == 0
    assert lib.memhip_bn_stats_workspace(64) == 128 * 2 * 64 * 4


@pytest.mark.parametrize("case", list(CASES) + ["bench"])
def test_plan_of_the_tested_shapes(case):
    from mem_amd import ops
    B, Cin, C, K, h, w = CASES.get(case, (16, 768, 256, 11, 32, 32))
    p = ops.bnhead_plan(B, C, K, h, w)
    print(case, {n: getattr(p, n) for n, _ in p._fields_})
    R = B * h * w
    assert p.R == R and p.block == 256 and p.kp == (K + 7) // 8 * 8 >= K
    assert p.fwd_grid == min(-(-R // 32), 512) and p.apply_grid_x == -(-R // 32) and p.sums_grid_x == min(-(-R // 64), 128)
    assert p.sums_grid_y == p.apply_grid_y == C // 64
    assert p.fwd_lds_bytes == p.kp * C * 4
    assert 0 < max(p.fwd_lds_bytes, p.sums_lds_bytes, p.apply_lds_bytes) <= 64 * 1024
    assert p.slot_floats == 2 * C + K * C + K and p.ws_bytes == p.sums_grid_x * p.slot_floats * 4
    assert p.fold_grid * 256 >= p.slot_floats
    # the largest head the entry points accept still fits: the whole classifier weight is the forward's only LDS
    big = ops.bnhead_plan(1, 512, 32, 3, 3)
    assert big.fwd_lds_bytes == 64 * 1024 and max(big.sums_lds_bytes, big.apply_lds_bytes) <= 64 * 1024
    assert ops.bnhead_plan(0, C, K, h, w).R == 0                                                      # B == 0 is fine
    assert ops.bn_stats_chain(R) == -(-R // (32 * min(-(-R // 32), 128))) + 32 + min(-(-R // 32), 128)


def test_ctypes_mirrors_match_the_header(tmp_path):
    """sizeof / offsetof of memhip_bnhead_args_t and memhip_bnhead_plan_t as the host compiler lays them out"""
    import os
    import re
    import subprocess
    from mem_amd import ops
    from test_abi_layout_cpu import HEADER, _host_cc
    cc = _host_cc()
    assert cc is not None, "no host C compiler"
    mirrors = {"memhip_bnhead_args_t": ops.BnHeadArgs, "memhip_bnhead_plan_t": ops.BnHeadPlan}
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "memhip.h"', "int main(void) {"]
    for name, cls in mirrors.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f[0], name, f[0]) for f in cls._fields_]
    lines += ["  return 0;", "}"]
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    open(src, "w").write("\n".join(lines) + "\n")
    r = subprocess.run([cc, "-I", os.path.dirname(HEADER), src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    printed = dict(re.findall(r"^(\S+) (\d+)$", subprocess.run([exe], capture_output=True, text=True, check=True).stdout, re.M))
    for name, cls in mirrors.items():
        assert ctypes.sizeof(cls) == int(printed[name]), name
        for f in cls._fields_:
            assert getattr(cls, f[0]).offset == int(printed[name + "." + f[0]]), (name, f[0])
    # every field of the C structs is mirrored: the header's field names in declaration order
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for tag, cls in (("memhip_bnhead_args", ops.BnHeadArgs), ("memhip_bnhead_plan", ops.BnHeadPlan)):
        body = re.search(r"struct\s+%s\s*\{(.*?)\};" % tag, text, flags=re.S).group(1)
        names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
        assert names == [f[0] for f in cls._fields_], (tag, names)


# ---------------------------------------------------------------------------------------------- the torch arm
def _head(**kw):
    from mem_amd.seg_heads import FCNHead
    cfg = dict(in_channels=10, channels=6, num_classes=4, in_index=1, dropout_ratio=0.5, impl="torch")
    cfg.update(kw)
    return FCNHead(**cfg)


def _randomise(head, gen):
    with torch.no_grad():
        for n, p in head.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * (0.3 if "conv" in n else 1.0) + (1.0 if n.endswith("bn.weight") else 0.0))


@pytest.mark.parametrize("mode", ["train", "train_nodrop", "eval"])
def test_torch_arm_against_the_oracle_in_float64(mode):
    gen = torch.Generator().manual_seed(11)
    head = _head(dropout_ratio=0.0 if mode == "train_nodrop" else 0.5).double()
    _randomise(head, gen)
    bn = head.convs[0].bn
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(6, generator=gen) * 0.2)
        bn.running_var.copy_(torch.rand(6, generator=gen) + 0.5)
    B, h, w = 3, 5, 7
    x = torch.randn(B, 10, h, w, generator=gen, dtype=torch.float64, requires_grad=True)
    keep = (torch.rand(B, 6, generator=gen) < 0.5).double()
    head.train(mode != "eval")
    head.keep_mask = keep
    running = (bn.running_mean.clone(), bn.running_var.clone()) if mode == "eval" else None
    out = head((None, x))
    params = [head.convs[0].conv.weight, bn.weight, bn.bias, head.conv_seg.weight, head.conv_seg.bias]
    gout = torch.randn(out.shape, generator=gen, dtype=torch.float64)
    got = torch.autograd.grad(out, [x] + params, gout)
    leaves = [t.detach().clone().requires_grad_() for t in [x] + params]
    ref = oracle_head(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4].reshape(4, 6), leaves[5],
                      keep if mode == "train" else None, 0.5 if mode == "train" else 0.0, bn.eps, running)
    want = torch.autograd.grad(ref, leaves, gout)
    print(mode, "logits rel %.3e" % _rel(out.detach(), ref.detach()))
    assert out.dtype == torch.float64 and tuple(out.shape) == (B, 4, h, w) and _rel(out.detach(), ref.detach()) <= 1e-10
    for name, a, b in zip(["x", "conv", "gamma", "beta", "wcls", "bias"], got, want):
        print(mode, name, "rel %.3e" % _rel(a, b))
        assert _rel(a, b.reshape(a.shape)) <= 1e-10, name


def test_running_statistics_follow_batchnorm2d():
    gen = torch.Generator().manual_seed(12)
    head = _head(dropout_ratio=0.1).train()
    _randomise(head, gen)
    conv, bn = head.convs[0].conv, head.convs[0].bn
    ref = torch.nn.BatchNorm2d(6).train()
    for _ in range(2):
        x = torch.randn(3, 10, 5, 7, generator=gen) * 2.0 + 0.5
        head([None, x])
        ref(F.conv2d(x, conv.weight, None, padding=1).detach())
    print("running mean", bn.running_mean, "var", bn.running_var, "n", int(bn.num_batches_tracked))
    assert int(bn.num_batches_tracked) == 2 == int(ref.num_batches_tracked)
    assert torch.equal(bn.running_mean, ref.running_mean) and torch.equal(bn.running_var, ref.running_var)
    head.eval()
    before = (bn.running_mean.clone(), bn.running_var.clone())
    head([None, x])
    assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1]) and int(bn.num_batches_tracked) == 2


@pytest.mark.parametrize("impl", ["torch", "hip"])
def test_state_dict_keys_are_mmsegs(impl):
    from mem_amd.seg_heads import FCNHead
    dims = dict(in_channels=128, channels=64, num_classes=11)
    head = FCNHead(impl=impl, **dims)
    sd = head.state_dict()
    assert list(sd) == list(MMSEG_KEYS)
    theirs = {k: torch.full([dims.get(s, s) for s in shape], 0.25) if shape else torch.tensor(7) for k, shape in MMSEG_KEYS.items()}
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in theirs.items()}
    head.load_state_dict(theirs, strict=True)
    assert int(head.convs[0].bn.num_batches_tracked) == 7 and float(head.conv_seg.weight.detach().mean()) == 0.25
    fresh = FCNHead(impl=impl, **dims)
    assert float(fresh.conv_seg.bias.detach().abs().max()) == 0.0 and 0.005 < float(fresh.conv_seg.weight.detach().std()) < 0.02
    assert fresh.convs[0].conv.bias is None
    d = FCNHead(impl=impl)                                               # the reference's auxiliary head
    assert (d.in_channels, d.channels, d.num_classes, d.in_index, d.dropout_ratio, d.loss_decode.loss_weight) == (768, 256, 11, 2, 0.1, 0.4)
    assert d.loss_decode.ignore_index == 255 and d.align_corners is False


@pytest.mark.parametrize("kw", [dict(num_convs=2), dict(concat_input=True), dict(kernel_size=1), dict(dilation=6),
                                dict(class_weight=[1.0] * 11), dict(sampler=dict(type="OHEMPixelSampler"))])
def test_refused_arguments_raise_by_name(kw):
    from mem_amd.seg_heads import FCNHead
    with pytest.raises(NotImplementedError, match=next(iter(kw))):
        FCNHead(**kw)
    with pytest.raises(TypeError, match="bogus"):
        FCNHead(bogus=1)
    with pytest.raises(ValueError):
        FCNHead(impl="hip", channels=100)
    with pytest.raises(ValueError):
        FCNHead(impl="hip", num_classes=33)


def test_seg_model_joins_the_heads_losses():
    """SegModel's dict and the sites of the two heads' masks, with stand-in modules (no device)."""
    from mem_amd import ops
    from mem_amd.seg_heads import FCNHead, SegModel

    class Stub(torch.nn.Module):
        def forward(self, img):
            return (img, img * 2.0)

    class Head(FCNHead):
        def forward_train(self, inputs, seg_label):
            return {"loss_seg": self.forward(inputs).mean(), "acc_seg": torch.tensor(50.0)}

    dec, aux = Head(impl="torch", in_channels=10, channels=6, num_classes=4, in_index=1), Head(impl="torch", in_channels=10, channels=6, num_classes=4, in_index=0)
    m = SegModel(Stub(), dec, aux)
    x = torch.randn(2, 10, 5, 7)
    out = m.forward_train(x, None)
    assert sorted(out) == ["aux.acc_seg", "aux.loss_seg", "decode.acc_seg", "decode.loss_seg"]
    assert (dec.dropout_site, aux.dropout_site) == (ops.DROPOUT_SITE_HEAD, ops.DROPOUT_SITE_HEAD + 1)
    assert ops.DROPOUT_SITE_HEAD > 2 * 10 ** 6                          # clear of every trunk site 0 .. 2 depth
    m.eval()
    assert tuple(m.encode_decode(x).shape) == (2, 4, 5, 7) and torch.equal(m(x), dec.forward_test((x, x * 2.0)))
    assert any(k.startswith("decode_head.convs.0.conv") for k in m.state_dict()) and any(k.startswith("auxiliary_head.") for k in m.state_dict())
