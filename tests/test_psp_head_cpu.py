"""-m "not gpu": the PSP decode head without a device -- the pool bins against torch's adaptive average pooling, the validation
and the plan of the pyramid-pooling entry points (host arithmetic), PSPHead(impl="torch") in float64 against a hand-written
expression of the same layers, the state-dict keys against mmseg's, and the refused arguments.

The cases, the states, the float64 expressions of the five kernels and ``oracle_psp`` serve tests/test_psp_head_gpu.py too; the
inputs of its per-kernel tests are checked here for the condition those tests put on them (hardly any ReLU gate within fp32
rounding of zero)."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from test_seg_head_cpu import oracle_head

EINVAL = -1
FAKE = 0x10000            # a non-null, 16-byte aligned address: validation never dereferences a pointer
U = 2.0 ** -24            # unit roundoff of fp32
# (B, Cin, C, K, h, w, pool scales): the cases of the GPU tests
CASES = {"P1": (4, 64, 64, 3, 7, 7, (1, 2, 3, 6)),        # the level-3 map at 224^2: every scale ragged, bins overlap, 6 on 7
         "P2": (4, 128, 128, 19, 6, 10, (1, 2, 3, 6)),    # s == h: an identity axis (all w1 == 0); ragged along w; two channel tiles
         "P3": (3, 768, 512, 11, 7, 10, (1, 2, 3, 6)),    # the reference's channel counts: the bottleneck is 9 x 2816 deep
         "P4": (4, 64, 64, 3, 8, 8, (2, 4)),              # two scales, exact bins that do not overlap
         "P5": (2, 64, 64, 3, 6, 6, (6,)),                # pooling and resize are identities
         "BIG": (2, 64, 64, 3, 40, 41, (1, 2, 3, 6))}     # bins of up to 1640 pixels, more tiles than workgroups: per kernel only
CALLS = ["memhip_ppm_pool", "memhip_ppm_concat_fwd", "memhip_ppm_concat_bwd_sums", "memhip_ppm_bwd_apply", "memhip_ppm_dmap"]


def mmseg_keys(n):
    """mmseg 0.30 PSPHead's state dict: key -> shape in terms of the constructor's arguments"""
    keys = {"conv_seg.weight": ("num_classes", "channels", 1, 1), "conv_seg.bias": ("num_classes",),
            "bottleneck.conv.weight": ("channels", "cat", 3, 3)}
    for pre in ["bottleneck.bn."] + ["psp_modules.%d.1.bn." % i for i in range(n)]:
        keys.update({pre + "weight": ("channels",), pre + "bias": ("channels",), pre + "running_mean": ("channels",),
                     pre + "running_var": ("channels",), pre + "num_batches_tracked": ()})
    keys.update({"psp_modules.%d.1.conv.weight" % i: ("channels", "in_channels", 1, 1) for i in range(n)})
    return keys


def param_names(n):
    """the parameters of a PSPHead in the order the tests report them"""
    names = []
    for i in range(n):
        names += ["psp_modules.%d.1.conv.weight" % i, "psp_modules.%d.1.bn.weight" % i, "psp_modules.%d.1.bn.bias" % i]
    return names + ["bottleneck.conv.weight", "bottleneck.bn.weight", "bottleneck.bn.bias", "conv_seg.weight", "conv_seg.bias"]


# ---------------------------------------------------------------------------------------------- float64 expressions
def pool_matrix(n, s):
    """A f64 [s, n]: 1 / count on the pixels of bin i = [floor(i n / s), ceil((i + 1) n / s)), written out here"""
    A = torch.zeros(s, n, dtype=torch.float64)
    for i in range(s):
        a, b = (i * n) // s, -((-(i + 1) * n) // s)
        A[i, a:b] = 1.0 / (b - a)
    return A


def resize_matrix(n_in, n_out, align_corners=False, table=None):
    """M f64 [out, in] of torch's bilinear resize along one axis; ``table`` = (i0, w1, ..) of ops.seg_axis_table: the fp32
    weights the kernels read, else the formula in float64"""
    M = torch.zeros(n_out, n_in, dtype=torch.float64)
    for y in range(n_out):
        if table is not None:
            a, w1 = int(table[0][y]), float(table[1][y])
        else:
            if align_corners:
                src = y * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
            else:
                src = max((y + 0.5) * n_in / n_out - 0.5, 0.0)
            a = min(int(src), n_in - 1)
            w1 = src - a
        M[y, a] += 1.0 - w1
        M[y, min(a + 1, n_in - 1)] += w1
    return M


def oracle_psp(x, psp, bott, wcls, bcls, scales, keep=None, p=0.0, eps=1e-5, running=None, align_corners=False):
    """mmseg's PSPHead by hand, any dtype, differentiable: per scale the mean over the bins, a 1x1 convolution, batch norm
    (batch statistics with the biased variance, or ``running`` = [(mean, var)] per branch and for the bottleneck last), ReLU,
    the bilinear resize; the concat; ``oracle_head`` for the bottleneck and ``cls_seg``.  psp = [(w [C, Cin], gamma, beta)],
    bott = (w [C, Cin + n C, 3, 3], gamma, beta)."""
    B, Cin, h, w = x.shape
    outs = [x]
    for i, (s, (wi, ga, be)) in enumerate(zip(scales, psp)):
        Ay, Ax = pool_matrix(h, s).to(x.dtype), pool_matrix(w, s).to(x.dtype)
        y = torch.einsum("oc,bcij->boij", wi, torch.einsum("iy,bcyx,jx->bcij", Ay, x, Ax))
        if running is None:
            mean = y.mean(dim=(0, 2, 3))
            var = ((y - mean[None, :, None, None]) ** 2).mean(dim=(0, 2, 3))
        else:
            mean, var = running[i]
        z = torch.clamp(ga[None, :, None, None] * (y - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + eps)
                        + be[None, :, None, None], min=0.0)
        My, Mx = resize_matrix(s, h, align_corners).to(x.dtype), resize_matrix(s, w, align_corners).to(x.dtype)
        outs.append(torch.einsum("yi,bcij,xj->bcyx", My, z, Mx))
    return oracle_head(torch.cat(outs, 1), bott[0], bott[1], bott[2], wcls, bcls, keep, p, eps, None if running is None else running[-1])


def state(case, seed=0):
    """x f32 of bf16 values, a state dict with bf16-valued convolution weights and non-trivial running statistics, a logit
    gradient"""
    B, Cin, C, K, h, w, scales = CASES[case]
    n = len(scales)
    gen = torch.Generator().manual_seed(2000 + seed + sum(map(ord, case)))
    x = (torch.randn(B, Cin, h, w, generator=gen) * 1.5).to(torch.bfloat16).float()
    sd = {}

    def bn(pre):
        sd.update({pre + "weight": 1.0 + 0.3 * torch.randn(C, generator=gen), pre + "bias": 0.3 * torch.randn(C, generator=gen),
                   pre + "running_mean": 0.2 * torch.randn(C, generator=gen), pre + "running_var": 0.5 + torch.rand(C, generator=gen),
                   pre + "num_batches_tracked": torch.tensor(3)})

    for i in range(n):
        sd["psp_modules.%d.1.conv.weight" % i] = (torch.randn(C, Cin, 1, 1, generator=gen) * (2.0 / Cin) ** 0.5).to(torch.bfloat16).float()
        bn("psp_modules.%d.1.bn." % i)
    ct = Cin + n * C
    sd["bottleneck.conv.weight"] = (torch.randn(C, ct, 3, 3, generator=gen) * (2.0 / (9 * ct)) ** 0.5).to(torch.bfloat16).float()
    bn("bottleneck.bn.")
    sd["conv_seg.weight"] = torch.randn(K, C, 1, 1, generator=gen) * (1.0 / C) ** 0.5
    sd["conv_seg.bias"] = 0.1 * torch.randn(K, generator=gen)
    gout = torch.randn(B, K, h, w, generator=gen)
    return x, sd, gout


def oracle_of_state(x, sd, scales, keep=None, p=0.0, train=True):
    """oracle_psp fed the tensors of a state dict (any dtype: that of x)"""
    n, t = len(scales), x.dtype
    K, C = sd["conv_seg.weight"].shape[:2]
    psp = [(sd["psp_modules.%d.1.conv.weight" % i].to(t).reshape(C, -1), sd["psp_modules.%d.1.bn.weight" % i].to(t),
            sd["psp_modules.%d.1.bn.bias" % i].to(t)) for i in range(n)]
    bott = (sd["bottleneck.conv.weight"].to(t), sd["bottleneck.bn.weight"].to(t), sd["bottleneck.bn.bias"].to(t))
    running = None
    if not train:
        running = [(sd[pre + "running_mean"].to(t), sd[pre + "running_var"].to(t))
                   for pre in ["psp_modules.%d.1.bn." % i for i in range(n)] + ["bottleneck.bn."]]
    return oracle_psp(x, psp, bott, sd["conv_seg.weight"].to(t).reshape(K, C), sd["conv_seg.bias"].to(t), scales, keep, p, 1e-5, running)


# ---------------------------------------------------------------------------------------------- the five kernels in float64
@functools.lru_cache(maxsize=None)
def kernel_inputs(case):
    """What the per-kernel tests store on the device, on the CPU: every tensor a kernel reads, drawn independently (a kernel is
    tested on its own stored inputs, not on its predecessor's output).  bf16 tensors hold bf16 values."""
    B, Cin, C, K, h, w, scales = CASES[case]
    n = len(scales)
    gen = torch.Generator().manual_seed(4242 + sum(map(ord, case)))
    bf = lambda *shape, scale=1.0, shift=0.0: (torch.randn(*shape, generator=gen) * scale + shift).to(torch.bfloat16)
    return dict(x=torch.randn(B, Cin, h, w, generator=gen) * 1.5,
                Y=[bf(B, s, s, C, scale=1.5, shift=0.3) for s in scales],
                mean=0.3 + 0.2 * torch.randn(n, C, generator=gen), rstd=0.5 + torch.rand(n, C, generator=gen),
                gamma=1.0 + 0.3 * torch.randn(n, C, generator=gen), beta=0.3 * torch.randn(n, C, generator=gen),
                dxcat=bf(B, h, w, Cin + n * C),
                g=[torch.randn(B * s * s, C, generator=gen) for s in scales], tot=torch.randn(n, 2, C, generator=gen),
                inv_n=[1.0 / (B * s * s) for s in scales],
                dP=[bf(B, s, s, Cin) for s in scales])


def bn_terms(inp, i):
    """xhat, u, the magnitude of xhat's terms and of u's terms, the gates either way; f64 [B, s, s, C] of scale i"""
    y, m, rs = inp["Y"][i].double(), inp["mean"][i].double(), inp["rstd"][i].double()
    ga, be = inp["gamma"][i].double(), inp["beta"][i].double()
    xh = (y - m) * rs
    u = ga * xh + be
    mag_xh = (y.abs() + m.abs()) * rs
    mag_u = ga.abs() * mag_xh + be.abs()
    amb = (u.abs() < 2.0 ** -20 * mag_u).double()         # within fp32 rounding of zero: the gate may fall either way
    return xh, u, mag_xh, mag_u, amb


def tables_of(case, align_corners=False):
    """per scale (My [h, s], Mx [w, s]) from the fp32 tables the kernels read, and the tables' lo / hi ranges"""
    from mem_amd import ops
    B, Cin, C, K, h, w, scales = CASES[case]
    out = []
    for s in scales:
        ty, tx = ops.seg_axis_table(s, h, align_corners), ops.seg_axis_table(s, w, align_corners)
        out.append((resize_matrix(s, h, table=ty), resize_matrix(s, w, table=tx), ty, tx))
    return out


# ---------------------------------------------------------------------------------------------- the pool bins
def test_bins_against_adaptive_avg_pool2d():
    """one-hot maps: the pooled value of bin i for the map with a one at pixel j is (j in bin i) / count(bin i)"""
    from mem_amd import ops
    checked = 0
    for n in range(1, 42):
        eye = torch.eye(n, dtype=torch.float64)
        for s in range(1, min(n, 8) + 1):
            start, end = ops.ppm_bins(n, s)
            want = F.adaptive_avg_pool2d(eye.view(n, 1, n, 1), (s, 1)).view(n, s)          # [pixel of the one, bin]
            member = torch.tensor([[start[i] <= j < end[i] for i in range(s)] for j in range(n)])
            count = torch.tensor([float(end[i] - start[i]) for i in range(s)], dtype=torch.float64)
            assert torch.equal(want, member.double() / count), (n, s)
            assert torch.equal(pool_matrix(n, s), want.t().contiguous()), (n, s)            # the tests' own expression too
            per_pixel = member.sum(1)
            assert int(per_pixel.min()) >= 1 and int(per_pixel.max()) <= 2, (n, s)          # at most two bins per axis
            assert start[0] == 0 and end[-1] == n and all(end[i] > start[i] for i in range(s))
            checked += 1
    assert checked == sum(min(n, 8) for n in range(1, 42))
    from mem_amd._lib import lib
    assert lib.memhip_ppm_bins(3, 4, FAKE, FAKE) == EINVAL and b"s=4" in lib.memhip_last_error()
    assert lib.memhip_ppm_bins(7, 6, None, FAKE) == EINVAL and b"null" in lib.memhip_last_error()


# ---------------------------------------------------------------------------------------------- validation and plan
def _args(ops, B=4, Cin=64, C=64, h=7, w=7, scales=(1, 2, 3, 6), **kw):
    four = lambda v: [v] * len(scales) if len(scales) <= 4 else [v] * 4
    fields = dict(map=FAKE, P=four(FAKE), Y=four(FAKE), mean=FAKE, rstd=FAKE, gamma=FAKE, beta=FAKE, xcat=FAKE, dxcat=FAKE, g=four(FAKE),
                  sums=FAKE, tot=FAKE, inv_n=four(0.5), dY=four(FAKE), dP=four(FAKE), dmap=FAKE)
    fields.update({k: four(FAKE) for k in ("y_i0", "y_w1", "y_lo", "y_hi", "x_i0", "x_w1", "x_lo", "x_hi")})
    fields.update(kw)
    return ops.ppm_args(B, Cin, C, h, w, scales, **fields)


BAD = [("Cin % 64", dict(Cin=96), b"Cin=96"), ("C % 64", dict(C=96), b"C=96"), ("C = 576", dict(C=576), b"C=576"),
       ("no scale", dict(scales=()), b"n=0"), ("five scales", dict(scales=(1, 2, 3, 4, 5)), b"n=5"),
       ("scale 9", dict(scales=(1, 9), h=12, w=12), b"scale 9"), ("scale 0", dict(scales=(0, 2)), b"scale 0"),
       ("scale above the map", dict(scales=(1, 2, 3, 6), h=5, w=7), b"scale 6 on a map of 5x7"), ("h = 0", dict(h=0), b"h=0"),
       ("B < 0", dict(B=-1), b"B=-1"), ("too many bins", dict(scales=(8, 8, 8, 8), h=8, w=8), b"LDS")]


@pytest.mark.parametrize("name,kw,word", BAD, ids=[b[0] for b in BAD])
def test_bad_shapes_are_rejected_before_any_launch(name, kw, word):
    from mem_amd import ops
    from mem_amd._lib import lib
    a = _args(ops, **kw)
    plan = ops.PpmPlan()
    rc_plan = lib.memhip_ppm_plan(ctypes.byref(a), ctypes.byref(plan))
    msg_plan = lib.memhip_last_error()
    for call in CALLS:
        rc = getattr(lib, call)(ctypes.byref(a), None)
        msg = lib.memhip_last_error()
        print(name, call, rc, rc_plan, msg)
        assert rc == EINVAL == rc_plan and word in msg and msg == msg_plan


NULLS = [("memhip_ppm_pool", "map", None), ("memhip_ppm_pool", "P", 2), ("memhip_ppm_concat_fwd", "map", None),
         ("memhip_ppm_concat_fwd", "Y", 0), ("memhip_ppm_concat_fwd", "rstd", None), ("memhip_ppm_concat_fwd", "xcat", None),
         ("memhip_ppm_concat_fwd", "x_w1", 3), ("memhip_ppm_concat_bwd_sums", "dxcat", None), ("memhip_ppm_concat_bwd_sums", "g", 1),
         ("memhip_ppm_concat_bwd_sums", "sums", None), ("memhip_ppm_concat_bwd_sums", "y_lo", 0), ("memhip_ppm_bwd_apply", "dY", 3),
         ("memhip_ppm_bwd_apply", "g", 0), ("memhip_ppm_bwd_apply", "gamma", None), ("memhip_ppm_dmap", "dP", 2),
         ("memhip_ppm_dmap", "dmap", None), ("memhip_ppm_dmap", "dxcat", None)]


@pytest.mark.parametrize("call,field,slot", NULLS)
def test_a_null_required_pointer_is_rejected(call, field, slot):
    from mem_amd import ops
    from mem_amd._lib import lib
    value = None if slot is None else [None if i == slot else FAKE for i in range(4)]
    rc = getattr(lib, call)(ctypes.byref(_args(ops, **{field: value})), None)
    print(call, field, slot, rc, lib.memhip_last_error())
    assert rc == EINVAL and b"null" in lib.memhip_last_error()
    assert getattr(lib, call)(None, None) == EINVAL
    # the plan takes the same struct with its pointers missing
    plan = ops.PpmPlan()
    assert lib.memhip_ppm_plan(ctypes.byref(_args(ops, **{field: value})), ctypes.byref(plan)) == 0


def test_misaligned_pointers_bad_inv_n_and_an_empty_batch():
    from mem_amd import ops
    from mem_amd._lib import lib
    assert lib.memhip_ppm_pool(ctypes.byref(_args(ops, P=[FAKE, FAKE + 2, FAKE, FAKE])), None) == EINVAL and b"aligned" in lib.memhip_last_error()
    assert lib.memhip_ppm_concat_fwd(ctypes.byref(_args(ops, xcat=FAKE + 8)), None) == EINVAL and b"aligned" in lib.memhip_last_error()
    assert lib.memhip_ppm_concat_fwd(ctypes.byref(_args(ops, mean=FAKE + 4)), None) == EINVAL and b"aligned" in lib.memhip_last_error()
    assert lib.memhip_ppm_bwd_apply(ctypes.byref(_args(ops, inv_n=[0.5, 0.0, 0.5, 0.5])), None) == EINVAL and b"inv_n[1]" in lib.memhip_last_error()
    assert lib.memhip_ppm_bwd_apply(ctypes.byref(_args(ops, tot=None, inv_n=[0.0] * 4, B=0)), None) == 0
    empty = ops.ppm_args(0, 64, 64, 7, 7, (1, 2, 3, 6))                                        # B == 0: nothing is read
    for call in CALLS:
        assert getattr(lib, call)(ctypes.byref(empty), None) == 0, call
    assert ops.ppm_plan(0, 64, 64, 7, 7, (1, 2, 3, 6)).R == 0


@pytest.mark.parametrize("case", list(CASES) + ["bench"])
def test_plan_of_the_tested_shapes(case):
    from mem_amd import ops
    B, Cin, C, K, h, w, scales = CASES.get(case, (16, 768, 512, 11, 14, 20, (1, 2, 3, 6)))
    n = len(scales)
    p = ops.ppm_plan(B, Cin, C, h, w, scales)
    print(case, {f: (list(getattr(p, f)) if hasattr(getattr(p, f), "__len__") else getattr(p, f)) for f, _ in p._fields_})
    R = B * h * w
    assert p.R == R and p.block == 256 and p.ct == Cin + n * C and p.bins == sum(s * s for s in scales) and p.ws_bytes == 0
    assert list(p.rows)[:n] == [B * s * s for s in scales]
    tiles = [-(-B * s * s // 32) for s in scales]
    assert list(p.row_tile0)[:n] == [sum(tiles[:i]) for i in range(n)] and p.gather_grid_x == sum(tiles)
    assert p.pool_grid == B * Cin // 64 and p.pool_lds_bytes == 64 * 65 * 4 + p.bins * (256 + 16) <= 64 * 1024
    assert p.concat_grid_x == p.dmap_grid_x == -(-R // 64) and p.concat_grid_y == Cin // 64 + n * C // 64 and p.dmap_grid_y == Cin // 64
    assert p.gather_grid_y == p.sums_grid_y == C // 64 and p.sums_grid_x == n and p.tile_lds_bytes == 64 * 65 * 4
    # the largest set of distinct scales still fits the pool's LDS
    assert ops.ppm_plan(1, 64, 64, 8, 8, (5, 6, 7, 8)).pool_lds_bytes <= 64 * 1024


def test_ctypes_mirrors_match_the_header(tmp_path):
    """sizeof / offsetof of memhip_ppm_args_t and memhip_ppm_plan_t as the host compiler lays them out"""
    import os
    import re
    import subprocess
    from mem_amd import ops
    from test_abi_layout_cpu import HEADER, _host_cc
    cc = _host_cc()
    assert cc is not None, "no host C compiler"
    mirrors = {"memhip_ppm_args_t": ops.PpmArgs, "memhip_ppm_plan_t": ops.PpmPlan}
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
    for tag, cls in (("memhip_ppm_args", ops.PpmArgs), ("memhip_ppm_plan", ops.PpmPlan)):
        body = re.sub(r"\[[^\]]*\]", "", re.search(r"struct\s+%s\s*\{(.*?)\};" % tag, text, flags=re.S).group(1))
        names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
        assert names == [f[0] for f in cls._fields_], (tag, names)
    assert ops.PPM_MAX_SCALES == int(re.search(r"#define MEMHIP_PPM_MAX_SCALES (\d+)", text).group(1))
    assert ops.PPM_MAX_SCALE == int(re.search(r"#define MEMHIP_PPM_MAX_SCALE (\d+)", text).group(1))


# ---------------------------------------------------------------------------------------------- the torch arm
def _head(case, impl, sd=None, p=0.0, **kw):
    from mem_amd.seg_heads import PSPHead
    B, Cin, C, K, h, w, scales = CASES[case]
    head = PSPHead(in_channels=Cin, channels=C, num_classes=K, in_index=0, pool_scales=scales, dropout_ratio=p, impl=impl, **kw)
    if sd is not None:
        head.load_state_dict(sd, strict=True)
    return head


@pytest.mark.parametrize("case", ["P1", "P2", "P4", "P5"])
@pytest.mark.parametrize("train", [True, False])
def test_the_torch_arm_in_float64_is_the_handwritten_expression(case, train):
    B, Cin, C, K, h, w, scales = CASES[case]
    x, sd, gout = state(case)
    p = 0.25
    keep = (torch.rand(B, C, generator=torch.Generator().manual_seed(3)) > p).to(torch.uint8)
    head = _head(case, "torch", sd, p).double().train(train)
    head.keep_mask = keep
    names = param_names(len(scales))
    xa = x.double().requires_grad_()
    out = head((xa,))
    got = torch.autograd.grad(out, [xa] + [dict(head.named_parameters())[n] for n in names], gout.double())
    leaves = {n: sd[n].double().requires_grad_() for n in names}
    xb = x.double().requires_grad_()
    want_out = oracle_of_state(xb, {**sd, **leaves}, scales, keep if train else None, p if train else 0.0, train)
    want = torch.autograd.grad(want_out, [xb] + [leaves[n] for n in names], gout.double())
    e = float((out - want_out).detach().abs().max() / want_out.detach().abs().max())
    print(case, "train" if train else "eval", "logits rel %.2e" % e)
    assert e <= 1e-12
    for n, a, b in zip(["x"] + names, got, want):
        e = float((a - b.reshape(a.shape)).abs().max() / b.abs().max())
        print("  d %-30s rel %.2e" % (n, e))
        assert e <= 1e-9, n                               # (gates flip nowhere: both sides are float64 on the same values)
    if train:
        assert all(int(b) == 4 for k, b in head.state_dict().items() if k.endswith("num_batches_tracked"))


def test_state_dict_is_mmsegs_and_moves_between_the_arms():
    case = "P2"
    B, Cin, C, K, h, w, scales = CASES[case]
    dims = dict(in_channels=Cin, channels=C, num_classes=K, cat=Cin + len(scales) * C)
    want = {k: tuple(dims.get(d, d) for d in shape) for k, shape in mmseg_keys(len(scales)).items()}
    hip, tor = _head(case, "hip"), _head(case, "torch")
    for head in (hip, tor):
        got = {k: tuple(v.shape) for k, v in head.state_dict().items()}
        assert got == want, sorted(set(got) ^ set(want))
    x, sd, _ = state(case)
    assert set(sd) == set(want)
    hip.load_state_dict(sd, strict=True)
    tor.load_state_dict(hip.state_dict(), strict=True)
    hip2 = _head(case, "hip")
    hip2.load_state_dict(tor.state_dict(), strict=True)
    assert all(torch.equal(v, hip2.state_dict()[k]) for k, v in sd.items())
    # the entries of a UPerHead checkpoint's decode_head that are this head's: the same keys and shapes
    uper = {"decode_head." + k: v for k, v in sd.items()}
    uper["decode_head.fpn_bottleneck.conv.weight"] = torch.zeros(1)
    mine = {k[len("decode_head."):]: v for k, v in uper.items() if k.startswith(("decode_head.psp_modules.", "decode_head.bottleneck."))}
    missing, unexpected = _head(case, "hip").load_state_dict(mine, strict=False)
    assert sorted(missing) == ["conv_seg.bias", "conv_seg.weight"] and not unexpected
    assert isinstance(hip.psp_modules, torch.nn.ModuleList) and len(hip.psp_modules[0]) == 2
    assert hip.psp_modules[0][1].conv.bias is None and hip.bottleneck.conv.padding == (1, 1)


def test_refusals_by_name():
    from mem_amd.seg_heads import FCNHead, PSPHead, SegModel
    ok = dict(in_channels=64, channels=64, num_classes=3)
    for kw, exc, word in [(dict(in_channels=96), ValueError, "in_channels=96"), (dict(channels=96), ValueError, "channels=96"),
                          (dict(channels=576), ValueError, "channels=576"), (dict(num_classes=1), ValueError, "num_classes"),
                          (dict(num_classes=33), ValueError, "num_classes"), (dict(pool_scales=(1, 2, 3, 4, 6)), ValueError, "at most 4 pool_scales"),
                          (dict(pool_scales=(1, 9)), ValueError, "1 <= s <= 8"), (dict(pool_scales=(0, 2)), ValueError, "pool_scales"),
                          (dict(pool_scales=()), ValueError, "pool_scales"), (dict(class_weight=[1.0] * 3), NotImplementedError, "class_weight"),
                          (dict(sampler=dict(type="OHEMPixelSampler")), NotImplementedError, "sampler"),
                          (dict(norm_cfg=dict(type="SyncBN")), TypeError, "norm_cfg"), (dict(impl="triton"), ValueError, "impl"),
                          (dict(dropout_ratio=1.0), ValueError, "dropout_ratio")]:
        with pytest.raises(exc) as e:
            PSPHead(**{**ok, **kw})
        print(kw, "->", e.value)
        assert word in str(e.value)
    # the torch arm takes what mmseg takes
    wide = PSPHead(in_channels=24, channels=40, num_classes=150, pool_scales=(1, 2, 3, 6, 12), impl="torch", in_index=0).eval()
    assert wide((torch.randn(2, 24, 5, 4),)).shape == (2, 150, 5, 4)
    # at the call: no CPU fallback, and the map must not be smaller than the largest scale
    from mem_amd._lib import MemhipError
    head = PSPHead(**ok, in_index=0)
    with pytest.raises(MemhipError) as e:
        head((torch.randn(2, 64, 7, 7),))
    assert "PSPHead(impl='hip')" in str(e.value) and "no CPU fallback" in str(e.value)
    with pytest.raises(ValueError) as e:
        head.ppm.check(4, 5, 7, True)
    assert "pool_scales" in str(e.value) and "5x7" in str(e.value)
    with pytest.raises(ValueError) as e:
        head.ppm.check(1, 7, 7, True)                                                     # B s^2 == 1 at scale 1, no process group
    assert "more than 1 value per channel" in str(e.value)
    head.ppm.check(1, 7, 7, False)                                                        # eval(): running statistics, fine
    head.ppm.check(2, 7, 7, True)
    with pytest.raises(ValueError):                                                       # torch's batch norm, the same case
        PSPHead(**ok, in_index=0, impl="torch").train()((torch.randn(1, 64, 7, 7),))
    # SegModel takes it as decode_head, and gives each head its own Dropout2d site
    from mem_amd import ops
    m = SegModel(torch.nn.Identity(), PSPHead(**ok), auxiliary_head=FCNHead(**ok))
    assert (m.decode_head.dropout_site, m.auxiliary_head.dropout_site) == (ops.DROPOUT_SITE_HEAD, ops.DROPOUT_SITE_HEAD + 1)


def test_batch_vectors_stacked_is_batch_vectors_per_row():
    from mem_amd.syncbn import batch_vectors, batch_vectors_stacked
    gen = torch.Generator().manual_seed(1)
    C, counts = 8, [4.0, 16.0, 36.0]
    st = torch.stack([torch.stack([torch.full((C,), c), torch.randn(C, generator=gen) * c, (1.0 + torch.rand(C, generator=gen)) * 3 * c]) for c in counts])
    tags = []

    def reduce(v, tag):
        tags.append(tag)
        return v * 2.0

    a = [torch.nn.BatchNorm2d(C) for _ in counts]
    b = [torch.nn.BatchNorm2d(C) for _ in counts]
    mean, rstd, inv_n = batch_vectors_stacked(a, lambda: st.clone(), reduce)
    assert tags == ["stats"]
    for i, bn in enumerate(b):
        m, r, iv = batch_vectors(bn, lambda: st[i].clone(), reduce)
        assert torch.equal(m, mean[i]) and torch.equal(r, rstd[i]) and torch.equal(iv, inv_n[i])
        assert torch.equal(bn.running_mean, a[i].running_mean) and torch.equal(bn.running_var, a[i].running_var)
        assert int(a[i].num_batches_tracked) == 1
    for bn in a:
        bn.eval()
    tags.clear()
    mean, rstd, inv_n = batch_vectors_stacked(a, None, None)
    assert inv_n is None and torch.equal(mean[1], a[1].running_mean) and torch.equal(rstd[2], torch.rsqrt(a[2].running_var + a[2].eps))


# ---------------------------------------------------------------------------------------------- the inputs of the per-kernel tests
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_inputs_have_hardly_any_gate_at_zero(case):
    """the condition tests/test_psp_head_gpu.py puts on its inputs, in float64 alone: far below 1 % of the ReLU gates lie
    within fp32 rounding of zero (such a gate may fall either way, and its whole term joins the bounds it enters)"""
    inp = kernel_inputs(case)
    n_amb = n_all = 0
    for i in range(len(CASES[case][6])):
        amb = bn_terms(inp, i)[4]
        n_amb, n_all = n_amb + int(amb.sum()), n_all + amb.numel()
    print(case, "%d of %d gates within fp32 rounding of zero" % (n_amb, n_all))
    assert n_amb <= 1e-3 * n_all
