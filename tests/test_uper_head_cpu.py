"""-m "not gpu": the UPerNet decode head without a device -- the validation and the plan of the FPN entry points (host
arithmetic), the ctypes mirrors against the header, UPerHead(impl="torch") in float64 against a hand-written expression of the
same layers (``oracle_uper``, built from tests/test_psp_head_cpu.py's ``oracle_psp``, ``resize_matrix`` and
tests/test_seg_head_cpu.py's ``oracle_head``), the state-dict keys against mmseg's, and the refused arguments.

The cases, the states, ``kernel_inputs`` and ``bn_terms`` serve tests/test_uper_head_gpu.py too; the inputs of its per-kernel
tests are checked here for the condition those tests put on them (hardly any ReLU gate within fp32 rounding of zero)."""
import ctypes
import functools

import pytest
import torch

from test_psp_head_cpu import oracle_psp, resize_matrix
from test_seg_head_cpu import oracle_head

EINVAL = -1
FAKE = 0x10000            # a non-null, 16-byte aligned address: validation never dereferences a pointer
U = 2.0 ** -24            # unit roundoff of fp32
# (B, in_channels, C, K, level sizes, pool scales): the cases of the GPU tests
CASES = {"U1": (4, (64,) * 4, 64, 3, ((28, 28), (14, 14), (7, 7), (3, 3)), (1, 2, 3)),      # EvBEiT's sizes at 112^2: 3 -> 7 is no 2x step
         "U2": (3, (128, 64, 128, 64), 128, 19, ((12, 20), (6, 10), (3, 5), (3, 5)), (1, 2, 3)),   # two equal levels: identity tables
         "U3": (2, (768,) * 4, 512, 11, ((16, 16), (8, 8), (4, 4), (2, 2)), (1, 2)),         # the reference's channel counts
         "U4": (4, (64,) * 2, 64, 3, ((8, 8), (4, 4)), (2, 4)),                             # L = 2: no middle level
         "BIG": (2, (64,) * 4, 64, 3, ((40, 41), (20, 21), (10, 11), (5, 6)), (1, 2, 3))}   # ragged tiles, many groups: per kernel only
CALLS = ["memhip_fpn_topdown_fwd", "memhip_fpn_concat_fwd", "memhip_fpn_resize_bwd", "memhip_fpn_bn_bwd_sums", "memhip_fpn_bn_bwd_apply"]


def conv_modules(L, n):
    """the ConvModules of a UPerHead under mmseg's names, with the shape of their convolution weight"""
    mods = {"psp_modules.%d.1" % i: ("channels", "in_last", 1, 1) for i in range(n)}
    mods["bottleneck"] = ("channels", "psp_cat", 3, 3)
    mods.update({"lateral_convs.%d" % l: ("channels", "in_%d" % l, 1, 1) for l in range(L - 1)})
    mods.update({"fpn_convs.%d" % l: ("channels", "channels", 3, 3) for l in range(L - 1)})
    mods["fpn_bottleneck"] = ("channels", "fpn_cat", 3, 3)
    return mods


def mmseg_keys(L, n):
    """mmseg 0.30 UPerHead's state dict: key -> shape in terms of the constructor's arguments"""
    keys = {"conv_seg.weight": ("num_classes", "channels", 1, 1), "conv_seg.bias": ("num_classes",)}
    for pre, shape in conv_modules(L, n).items():
        keys[pre + ".conv.weight"] = shape
        keys.update({pre + ".bn.weight": ("channels",), pre + ".bn.bias": ("channels",), pre + ".bn.running_mean": ("channels",),
                     pre + ".bn.running_var": ("channels",), pre + ".bn.num_batches_tracked": ()})
    return keys


def dims_of(case):
    B, ins, C, K, sizes, scales = CASES[case]
    d = dict(channels=C, num_classes=K, in_last=ins[-1], psp_cat=ins[-1] + len(scales) * C, fpn_cat=len(ins) * C)
    d.update({"in_%d" % l: c for l, c in enumerate(ins)})
    return d


def param_names(L, n):
    """the parameters of a UPerHead in the order the tests report them"""
    names = []
    for pre in conv_modules(L, n):
        names += [pre + ".conv.weight", pre + ".bn.weight", pre + ".bn.bias"]
    return names + ["conv_seg.weight", "conv_seg.bias"]


# ---------------------------------------------------------------------------------------------- float64 expressions
def oracle_cm1(x, w, gamma, beta, eps=1e-5, running=None):
    """a 1x1 ConvModule by hand: x [B, Cin, h, w], w [C, Cin]"""
    y = torch.einsum("oc,bchw->bohw", w, x)
    if running is None:
        mean = y.mean(dim=(0, 2, 3))
        var = ((y - mean[None, :, None, None]) ** 2).mean(dim=(0, 2, 3))
    else:
        mean, var = running
    return torch.clamp(gamma[None, :, None, None] * (y - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + eps)
                       + beta[None, :, None, None], min=0.0)


def oracle_cm3(x, w, gamma, beta, eps=1e-5, running=None):
    """a 3x3 ConvModule: oracle_head with the identity as classifier"""
    C = w.shape[0]
    return oracle_head(x, w, gamma, beta, torch.eye(C, dtype=x.dtype), torch.zeros(C, dtype=x.dtype), None, 0.0, eps, running)


def resize2(z, size, align_corners=False):
    My, Mx = resize_matrix(z.shape[2], size[0], align_corners).to(z.dtype), resize_matrix(z.shape[3], size[1], align_corners).to(z.dtype)
    return torch.einsum("yi,bcij,xj->bcyx", My, z, Mx)


def oracle_uper(xs, sd, scales, keep=None, p=0.0, train=True, eps=1e-5, align_corners=False):
    """mmseg's UPerHead by hand from a state dict (any dtype: that of xs), differentiable"""
    L, n, t = len(xs), len(scales), xs[0].dtype
    g = lambda k: sd[k].to(t)
    run = lambda pre: None if train else (g(pre + ".bn.running_mean"), g(pre + ".bn.running_var"))
    cm = lambda pre: (g(pre + ".conv.weight"), g(pre + ".bn.weight"), g(pre + ".bn.bias"))
    C = sd["conv_seg.weight"].shape[1]
    lats = []
    for l in range(L - 1):
        w, ga, be = cm("lateral_convs.%d" % l)
        lats.append(oracle_cm1(xs[l], w.reshape(C, -1), ga, be, eps, run("lateral_convs.%d" % l)))
    psp = [(cm("psp_modules.%d.1" % i)[0].reshape(C, -1),) + cm("psp_modules.%d.1" % i)[1:] for i in range(n)]
    running = None if train else [run("psp_modules.%d.1" % i) for i in range(n)] + [run("bottleneck")]
    lats.append(oracle_psp(xs[-1], psp, cm("bottleneck"), torch.eye(C, dtype=t), torch.zeros(C, dtype=t), scales, None, 0.0, eps, running,
                           align_corners))
    for l in range(L - 1, 0, -1):
        lats[l - 1] = lats[l - 1] + resize2(lats[l], lats[l - 1].shape[2:], align_corners)
    outs = [oracle_cm3(lats[l], *cm("fpn_convs.%d" % l), eps, run("fpn_convs.%d" % l)) for l in range(L - 1)] + [lats[-1]]
    outs = [outs[0]] + [resize2(o, outs[0].shape[2:], align_corners) for o in outs[1:]]
    K = sd["conv_seg.weight"].shape[0]
    return oracle_head(torch.cat(outs, 1), *cm("fpn_bottleneck"), g("conv_seg.weight").reshape(K, C), g("conv_seg.bias"), keep, p, eps,
                       run("fpn_bottleneck"))


@functools.lru_cache(maxsize=None)
def state(case, seed=0):
    """xs f32 of bf16 values, a state dict with bf16-valued convolution weights and non-trivial running statistics, a logit
    gradient"""
    B, ins, C, K, sizes, scales = CASES[case]
    dims = dims_of(case)
    gen = torch.Generator().manual_seed(3000 + seed + sum(map(ord, case)))
    xs = [(torch.randn(B, c, h, w, generator=gen) * 1.5).to(torch.bfloat16).float() for c, (h, w) in zip(ins, sizes)]
    sd = {}
    for pre, shape in conv_modules(len(ins), len(scales)).items():
        shape = tuple(dims.get(d, d) for d in shape)
        sd[pre + ".conv.weight"] = (torch.randn(shape, generator=gen) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5).to(torch.bfloat16).float()
        sd.update({pre + ".bn.weight": 1.0 + 0.3 * torch.randn(C, generator=gen), pre + ".bn.bias": 0.3 * torch.randn(C, generator=gen),
                   pre + ".bn.running_mean": 0.2 * torch.randn(C, generator=gen), pre + ".bn.running_var": 0.5 + torch.rand(C, generator=gen),
                   pre + ".bn.num_batches_tracked": torch.tensor(3)})
    sd["conv_seg.weight"] = torch.randn(K, C, 1, 1, generator=gen) * (1.0 / C) ** 0.5
    sd["conv_seg.bias"] = 0.1 * torch.randn(K, generator=gen)
    gout = torch.randn(B, K, sizes[0][0], sizes[0][1], generator=gen)
    return xs, sd, gout


# ---------------------------------------------------------------------------------------------- the inputs of the per-kernel tests
@functools.lru_cache(maxsize=None)
def kernel_inputs(case):
    """What the per-kernel tests store on the device, on the CPU: every tensor a kernel reads, drawn independently (a kernel is
    tested on its own stored inputs, not on its predecessor's output).  bf16 tensors hold bf16 values."""
    B, ins, C, K, sizes, scales = CASES[case]
    L = len(sizes)
    gen = torch.Generator().manual_seed(5151 + sum(map(ord, case)))
    bf = lambda *shape, scale=1.0, shift=0.0: (torch.randn(*shape, generator=gen) * scale + shift).to(torch.bfloat16)
    return dict(Y=[bf(B, h, w, C, scale=1.5, shift=0.3) for h, w in sizes],
                mean=0.3 + 0.2 * torch.randn(L, C, generator=gen), rstd=0.5 + torch.rand(L, C, generator=gen),
                gamma=1.0 + 0.3 * torch.randn(L, C, generator=gen), beta=0.3 * torch.randn(L, C, generator=gen),
                T=[bf(B, h, w, C, scale=1.5) for h, w in sizes],                          # a stored top-down sum per level
                dxcat=bf(B, sizes[0][0], sizes[0][1], L * C),
                own=[bf(B, h, w, C) for h, w in sizes],
                rows=[torch.randn(B * h * w, C, generator=gen) for h, w in sizes],       # fp32 rows per level
                tot=torch.randn(2, C, generator=gen), inv_n=[1.0 / (B * h * w) for h, w in sizes])


def bn_terms(inp, l):
    """xhat, u, the magnitude of xhat's terms and of u's terms, the ambiguous gates; f64 [B, h, w, C] of level l"""
    y, m, rs = inp["Y"][l].double(), inp["mean"][l].double(), inp["rstd"][l].double()
    ga, be = inp["gamma"][l].double(), inp["beta"][l].double()
    xh = (y - m) * rs
    u = ga * xh + be
    mag_xh = (y.abs() + m.abs()) * rs
    mag_u = ga.abs() * mag_xh + be.abs()
    amb = (u.abs() < 2.0 ** -20 * mag_u).double()         # within fp32 rounding of zero: the gate may fall either way
    return xh, u, mag_xh, mag_u, amb


def table_pair(n_in_hw, n_out_hw, align_corners=False):
    """(My [out, in], Mx [out, in], ty, tx) from the fp32 tables the kernels read"""
    from mem_amd import ops
    ty, tx = ops.seg_axis_table(n_in_hw[0], n_out_hw[0], align_corners), ops.seg_axis_table(n_in_hw[1], n_out_hw[1], align_corners)
    return resize_matrix(n_in_hw[0], n_out_hw[0], table=ty), resize_matrix(n_in_hw[1], n_out_hw[1], table=tx), ty, tx


@pytest.mark.parametrize("case", list(CASES))
def test_kernel_inputs_have_hardly_any_gate_at_zero(case):
    """the condition tests/test_uper_head_gpu.py puts on its inputs, in float64 alone: at most 1e-3 of the ReLU gates lie
    within fp32 rounding of zero (such a gate may fall either way, and its whole term joins the bounds it enters)"""
    inp = kernel_inputs(case)
    n_amb = n_all = 0
    for l in range(len(CASES[case][4])):
        amb = bn_terms(inp, l)[4]
        n_amb, n_all = n_amb + int(amb.sum()), n_all + amb.numel()
    print(case, "%d of %d gates within fp32 rounding of zero" % (n_amb, n_all))
    assert n_amb <= 1e-3 * n_all


# ---------------------------------------------------------------------------------------------- validation and plan
def _args(ops, B=4, C=64, sizes=((28, 28), (14, 14), (7, 7), (3, 3)), level=1, **kw):
    four = lambda v: [v] * 4
    fields = dict(Y=four(FAKE), mean=FAKE, rstd=FAKE, gamma=FAKE, beta=FAKE, src=FAKE, T=FAKE, xcat=FAKE, own=FAKE, dxcat=FAKE,
                  fine_rows=FAKE, slice=1, rows=FAKE, sums=FAKE, workspace=FAKE, workspace_bytes=1 << 30, tot=FAKE, inv_n=0.5, dY=FAKE)
    fields.update({k: four(FAKE) for k in ops._FPN_TABLES})
    fields.update(kw)
    return ops.fpn_args(B, C, sizes, level, **fields)


S4 = ((28, 28), (14, 14), (7, 7), (3, 3))
BAD = [("C % 64", dict(C=96), b"C=96"), ("C = 576", dict(C=576), b"C=576"), ("C = 0", dict(C=0), b"C=0"), ("B < 0", dict(B=-1), b"B=-1"),
       ("one level", dict(sizes=((8, 8),), level=0), b"L=1"), ("five levels", dict(sizes=S4 + ((1, 1),)), b"L=5"),
       ("h = 0", dict(sizes=((8, 8), (0, 4)), level=0), b"level 1: 0x4"),
       ("a level grows in h", dict(sizes=((8, 8), (4, 4), (5, 4)), level=0), b"level 2 of 5x4 above level 1 of 4x4"),
       ("a level grows in w", dict(sizes=((8, 8), (8, 9)), level=0), b"level 1 of 8x9 above level 0 of 8x8"),
       ("level = L", dict(sizes=((8, 8), (4, 4)), level=2), b"bad level 2"), ("level < 0", dict(level=-1), b"bad level -1"),
       ("too many pixels", dict(B=1 << 20, sizes=((64, 64), (1, 1)), level=0), b"too many pixels"),
       ("a small workspace", dict(workspace_bytes=128 * 2 * 64 * 4 - 1), b"workspace of")]


@pytest.mark.parametrize("name,kw,word", BAD, ids=[b[0] for b in BAD])
def test_bad_shapes_are_rejected_before_any_launch(name, kw, word):
    from mem_amd import ops
    from mem_amd._lib import lib
    a = _args(ops, **kw)
    plan = ops.FpnPlan()
    rc_plan = lib.memhip_fpn_plan(ctypes.byref(a), ctypes.byref(plan))
    msg_plan = lib.memhip_last_error()
    calls = ["memhip_fpn_bn_bwd_sums"] if name == "a small workspace" else CALLS      # (a field another call owns is ignored)
    for call in calls:
        rc = getattr(lib, call)(ctypes.byref(a), None)
        msg = lib.memhip_last_error()
        print(name, call, rc, rc_plan, msg)
        assert rc == EINVAL == rc_plan and word in msg and msg == msg_plan


# (call, field, slot of a per-level field or None, level, word)
NULLS = [("memhip_fpn_topdown_fwd", "Y", 1, 1, b"Y[1]"), ("memhip_fpn_topdown_fwd", "T", None, 1, b"T is null"),
         ("memhip_fpn_topdown_fwd", "gamma", None, 1, b"null"), ("memhip_fpn_topdown_fwd", "ty_i0", 1, 1, b"tables t of level 1"),
         ("memhip_fpn_topdown_fwd", "tx_w1", 0, 0, b"tables t of level 0"),
         ("memhip_fpn_topdown_fwd", "src", None, 1, b"null pointer (src) at level 1"),       # only level L - 2 may read Y in place of src
         ("memhip_fpn_concat_fwd", "Y", 3, 1, b"Y[3]"), ("memhip_fpn_concat_fwd", "xcat", None, 1, b"xcat"),
         ("memhip_fpn_concat_fwd", "cx_i0", 2, 1, b"tables c of level 2"), ("memhip_fpn_concat_fwd", "mean", None, 1, b"null"),
         ("memhip_fpn_resize_bwd", "rows", None, 1, b"rows"), ("memhip_fpn_resize_bwd", "cy_lo", 1, 1, b"tables c of level 1"),
         ("memhip_fpn_resize_bwd", "tx_hi", 0, 1, b"tables t of level 0"),
         ("memhip_fpn_bn_bwd_sums", "Y", 1, 1, b"Y[1]"), ("memhip_fpn_bn_bwd_sums", "rows", None, 1, b"rows"),
         ("memhip_fpn_bn_bwd_sums", "sums", None, 1, b"sums"), ("memhip_fpn_bn_bwd_sums", "workspace", None, 1, b"workspace"),
         ("memhip_fpn_bn_bwd_sums", "rstd", None, 1, b"null"),
         ("memhip_fpn_bn_bwd_apply", "dY", None, 1, b"dY"), ("memhip_fpn_bn_bwd_apply", "Y", 2, 2, b"Y[2]"),
         ("memhip_fpn_bn_bwd_apply", "rows", None, 1, b"rows"), ("memhip_fpn_bn_bwd_apply", "beta", None, 1, b"null")]


@pytest.mark.parametrize("call,field,slot,level,word", NULLS)
def test_a_null_required_pointer_is_rejected(call, field, slot, level, word):
    from mem_amd import ops
    from mem_amd._lib import lib
    value = None if slot is None else [None if i == slot else FAKE for i in range(4)]
    rc = getattr(lib, call)(ctypes.byref(_args(ops, level=level, **{field: value})), None)
    print(call, field, slot, rc, lib.memhip_last_error())
    assert rc == EINVAL and word in lib.memhip_last_error() and b"null" in lib.memhip_last_error()
    assert getattr(lib, call)(None, None) == EINVAL
    # the plan takes the same struct with its pointers missing
    plan = ops.FpnPlan()
    assert lib.memhip_fpn_plan(ctypes.byref(_args(ops, level=level, **{field: value})), ctypes.byref(plan)) == 0
    assert lib.memhip_fpn_plan(ctypes.byref(_args(ops)), None) == EINVAL


def test_the_rules_of_single_calls():
    """what only one call refuses: levels without a source, terms without a finer level, slices, misaligned pointers, inv_n"""
    from mem_amd import ops
    from mem_amd._lib import lib
    err = lib.memhip_last_error
    bad = lambda call, **kw: getattr(lib, call)(ctypes.byref(_args(ops, **kw)), None) == EINVAL
    assert bad("memhip_fpn_topdown_fwd", level=3) and b"coarsest level 3 has no source" in err()
    assert bad("memhip_fpn_topdown_fwd", level=2, src=None, Y=[FAKE, FAKE, FAKE, None]) and b"Y[3]" in err()
    assert bad("memhip_fpn_topdown_fwd", src=FAKE + 8) and b"src is not 16-byte aligned" in err()
    assert bad("memhip_fpn_topdown_fwd", T=FAKE + 2) and b"aligned" in err()
    assert bad("memhip_fpn_concat_fwd", xcat=FAKE + 8) and b"aligned" in err()
    assert bad("memhip_fpn_concat_fwd", mean=FAKE + 4) and b"aligned" in err()
    assert bad("memhip_fpn_concat_fwd", Y=[FAKE, FAKE + 2, FAKE, FAKE]) and b"Y[1]" in err()
    assert bad("memhip_fpn_resize_bwd", own=None, dxcat=None, fine_rows=None) and b"no term" in err()
    assert bad("memhip_fpn_resize_bwd", level=0) and b"fine_rows at level 0" in err()
    assert bad("memhip_fpn_resize_bwd", slice=4) and b"bad slice 4" in err()
    assert bad("memhip_fpn_resize_bwd", slice=-1) and b"bad slice -1" in err()
    assert bad("memhip_fpn_resize_bwd", own=FAKE + 8) and b"aligned" in err()
    assert bad("memhip_fpn_resize_bwd", rows=FAKE + 4) and b"aligned" in err()
    assert bad("memhip_fpn_bn_bwd_sums", workspace=FAKE + 8) and b"aligned" in err()
    assert bad("memhip_fpn_bn_bwd_sums", rows=FAKE + 8) and b"aligned" in err()
    assert bad("memhip_fpn_bn_bwd_apply", inv_n=0.0) and b"inv_n=0" in err()
    assert bad("memhip_fpn_bn_bwd_apply", inv_n=float("inf")) and b"inv_n" in err()
    assert bad("memhip_fpn_bn_bwd_apply", tot=FAKE + 4) and b"tot is not 16-byte aligned" in err()
    assert bad("memhip_fpn_bn_bwd_apply", dY=FAKE + 2) and b"aligned" in err()
    # a field another call owns is ignored: a bad slice and inv_n without tot mean nothing to the sums
    plan = ops.FpnPlan()
    assert lib.memhip_fpn_plan(ctypes.byref(_args(ops, slice=9, inv_n=0.0, src=None, own=None, dxcat=None, fine_rows=None)), ctypes.byref(plan)) == 0
    # B == 0: nothing is read, whatever the pointers
    empty = ops.fpn_args(0, 64, S4, 1)
    for call in CALLS:
        assert getattr(lib, call)(ctypes.byref(empty), None) == 0, call
    assert list(ops.fpn_plan(0, 64, S4).R) == [0, 0, 0, 0]


@pytest.mark.parametrize("case", list(CASES) + ["bench"])
def test_plan_of_the_tested_shapes(case):
    from mem_amd import ops
    B, ins, C, K, sizes, scales = CASES.get(case, (16, (768,) * 4, 512, 11, ((56, 56), (28, 28), (14, 14), (7, 7)), (1, 2, 3, 6)))
    L = len(sizes)
    p = ops.fpn_plan(B, C, sizes)
    print(case, {f: (list(getattr(p, f)) if hasattr(getattr(p, f), "__len__") else getattr(p, f)) for f, _ in p._fields_})
    R = [B * h * w for h, w in sizes]
    pad = lambda v: v + [0] * (4 - L)
    assert list(p.R) == pad(R) and p.block == 256 and p.ct == L * C and p.grid_y == C // 64
    assert p.concat_grid_x == -(-R[0] // 64) and p.concat_grid_y == L * C // 64
    assert list(p.topdown_grid_x) == pad([-(-r // 64) for r in R[:-1]] + [0])
    assert list(p.resize_grid_x) == pad([-(-r // 32) for r in R])
    assert list(p.sums_grid_x) == pad([min(-(-r // 32), 128) for r in R])
    assert list(p.apply_grid_x) == pad([-(-r // 64) for r in R])
    assert p.sums_lds_bytes == 2 * 32 * 64 * 4 and p.slot_floats == 2 * C and p.fold_grid == -(-2 * C // 256)
    assert p.ws_bytes == 128 * 2 * C * 4 == ops.fpn_sums_workspace(C, "cpu").numel() * 4
    if case == "U1":                                      # by hand: 4 x 784, 196, 49, 9 pixels
        assert list(p.R) == [3136, 784, 196, 36] and list(p.topdown_grid_x) == [49, 13, 4, 0] and list(p.resize_grid_x) == [98, 25, 7, 2]
        assert list(p.sums_grid_x) == [98, 25, 7, 2] and list(p.apply_grid_x) == [49, 13, 4, 1] and (p.concat_grid_x, p.concat_grid_y) == (49, 4)
        assert p.ws_bytes == 65536
    if case == "BIG":                                     # by hand: 2 x 1640, 420, 110, 30 pixels; the sums' groups are capped
        assert list(p.R) == [3280, 840, 220, 60] and list(p.topdown_grid_x) == [52, 14, 4, 0] and list(p.resize_grid_x) == [103, 27, 7, 2]
        assert list(p.sums_grid_x) == [103, 27, 7, 2] and list(p.apply_grid_x) == [52, 14, 4, 1] and (p.concat_grid_x, p.concat_grid_y) == (52, 4)
    if case == "bench":                                   # 16 x 3136 pixels at level 0: more rows than 32 x 128, the groups are capped
        assert list(p.sums_grid_x) == [128, 128, 98, 25]


def test_ctypes_mirrors_match_the_header(tmp_path):
    """sizeof / offsetof of memhip_fpn_args_t and memhip_fpn_plan_t as the host compiler lays them out"""
    import os
    import re
    import subprocess
    from mem_amd import ops
    from test_abi_layout_cpu import HEADER, _host_cc
    cc = _host_cc()
    assert cc is not None, "no host C compiler"
    mirrors = {"memhip_fpn_args_t": ops.FpnArgs, "memhip_fpn_plan_t": ops.FpnPlan}
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
    for tag, cls in (("memhip_fpn_args", ops.FpnArgs), ("memhip_fpn_plan", ops.FpnPlan)):
        body = re.sub(r"\[[^\]]*\]", "", re.search(r"struct\s+%s\s*\{(.*?)\};" % tag, text, flags=re.S).group(1))
        names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
        assert names == [f[0] for f in cls._fields_], (tag, names)
    assert ops.FPN_MAX_LEVELS == int(re.search(r"#define MEMHIP_FPN_MAX_LEVELS (\d+)", text).group(1))


# ---------------------------------------------------------------------------------------------- the torch arm
def _head(case, impl, sd=None, p=0.0, **kw):
    from mem_amd.seg_heads import UPerHead
    B, ins, C, K, sizes, scales = CASES[case]
    head = UPerHead(in_channels=ins, channels=C, num_classes=K, in_index=tuple(range(len(ins))), pool_scales=scales, dropout_ratio=p,
                    impl=impl, **kw)
    if sd is not None:
        head.load_state_dict(sd, strict=True)
    return head


@pytest.mark.parametrize("case", ["U1", "U2", "U4"])
@pytest.mark.parametrize("train", [True, False])
def test_the_torch_arm_in_float64_is_the_handwritten_expression(case, train):
    B, ins, C, K, sizes, scales = CASES[case]
    xs, sd, gout = state(case)
    p = 0.25
    keep = (torch.rand(B, C, generator=torch.Generator().manual_seed(3)) > p).to(torch.uint8)
    head = _head(case, "torch", sd, p).double().train(train)
    head.keep_mask = keep
    names = param_names(len(ins), len(scales))
    xa = [x.double().requires_grad_() for x in xs]
    out = head(tuple(xa))
    got = torch.autograd.grad(out, xa + [dict(head.named_parameters())[n] for n in names], gout.double())
    leaves = {n: sd[n].double().requires_grad_() for n in names}
    xb = [x.double().requires_grad_() for x in xs]
    want_out = oracle_uper(xb, {**sd, **leaves}, scales, keep if train else None, p if train else 0.0, train)
    want = torch.autograd.grad(want_out, xb + [leaves[n] for n in names], gout.double())
    e = float((out - want_out).detach().abs().max() / want_out.detach().abs().max())
    print(case, "train" if train else "eval", "logits rel %.2e" % e)
    assert e <= 1e-10
    for n, a, b in zip(["x%d" % l for l in range(len(ins))] + names, got, want):
        e = float((a - b.reshape(a.shape)).abs().max() / b.abs().max())
        print("  d %-32s rel %.2e" % (n, e))
        assert e <= 1e-10, n                              # (gates flip nowhere: both sides are float64 on the same values)
    if train:
        assert all(int(b) == 4 for k, b in head.state_dict().items() if k.endswith("num_batches_tracked"))


def test_state_dict_is_mmsegs_and_moves_between_the_arms():
    case = "U2"
    B, ins, C, K, sizes, scales = CASES[case]
    dims = dims_of(case)
    want = {k: tuple(dims.get(d, d) for d in shape) for k, shape in mmseg_keys(len(ins), len(scales)).items()}
    hip, tor = _head(case, "hip"), _head(case, "torch")
    for head in (hip, tor):
        got = {k: tuple(v.shape) for k, v in head.state_dict().items()}
        assert got == want, sorted(set(got) ^ set(want))
    xs, sd, _ = state(case)
    assert set(sd) == set(want) and len(want) == 2 + 6 * (len(scales) + 1 + 2 * (len(ins) - 1) + 1)
    hip.load_state_dict(sd, strict=True)
    tor.load_state_dict(hip.state_dict(), strict=True)
    hip2 = _head(case, "hip")
    hip2.load_state_dict(tor.state_dict(), strict=True)
    assert all(torch.equal(v, hip2.state_dict()[k]) for k, v in sd.items())
    # a reference checkpoint's decode_head.* is this head's state dict, key for key
    ckpt = {"decode_head." + k: v for k, v in sd.items()}
    _head(case, "hip").load_state_dict({k[len("decode_head."):]: v for k, v in ckpt.items()}, strict=True)
    # a PSPHead's pyramid entries are the UPerHead's, unchanged
    from mem_amd.seg_heads import PSPHead
    psp = PSPHead(in_channels=ins[-1], channels=C, num_classes=K, pool_scales=scales, impl="torch")
    mine = {k: v for k, v in psp.state_dict().items() if k.startswith(("psp_modules.", "bottleneck."))}
    missing, unexpected = _head(case, "hip").load_state_dict(mine, strict=False)
    assert not unexpected and not [k for k in missing if k.startswith(("psp_modules.", "bottleneck."))]
    assert isinstance(hip.lateral_convs, torch.nn.ModuleList) and hip.lateral_convs[0].conv.kernel_size == (1, 1)
    assert hip.fpn_convs[0].conv.padding == (1, 1) and hip.fpn_bottleneck.conv.bias is None


def test_refusals_by_name():
    from mem_amd.seg_heads import FCNHead, SegModel, UPerHead
    ok = dict(in_channels=(64,) * 4, channels=64, num_classes=3)
    for kw, exc, word in [(dict(in_channels=(64, 96, 64, 64)), ValueError, "in_channels=96"), (dict(channels=96), ValueError, "channels=96"),
                          (dict(channels=576), ValueError, "channels=576"), (dict(num_classes=1), ValueError, "num_classes"),
                          (dict(num_classes=33), ValueError, "num_classes"), (dict(in_index=(0, 1, 2)), ValueError, "len(in_index)=3"),
                          (dict(in_channels=(64,), in_index=(0,)), ValueError, "2 <= levels <= 4"),
                          (dict(in_channels=(64,) * 5, in_index=(0, 1, 2, 3, 4)), ValueError, "2 <= levels <= 4"),
                          (dict(pool_scales=(1, 2, 3, 4, 6)), ValueError, "at most 4 pool_scales"),
                          (dict(pool_scales=(1, 9)), ValueError, "1 <= s <= 8"), (dict(pool_scales=(0, 2)), ValueError, "pool_scales"),
                          (dict(pool_scales=()), ValueError, "pool_scales"), (dict(class_weight=[1.0] * 3), NotImplementedError, "class_weight"),
                          (dict(sampler=dict(type="OHEMPixelSampler")), NotImplementedError, "sampler"),
                          (dict(norm_cfg=dict(type="SyncBN")), TypeError, "norm_cfg"), (dict(impl="triton"), ValueError, "impl"),
                          (dict(dropout_ratio=1.0), ValueError, "dropout_ratio")]:
        with pytest.raises(exc) as e:
            UPerHead(**{**ok, **kw})
        print(kw, "->", e.value)
        assert word in str(e.value)
    # the torch arm takes what mmseg takes: any widths, five levels, sizes in any order
    wide = UPerHead(in_channels=(24, 8, 8, 8, 8), channels=40, num_classes=150, in_index=(0, 1, 2, 3, 4), pool_scales=(1, 2, 3, 6, 12),
                    impl="torch").eval()
    assert wide([torch.randn(2, c, s, s) for c, s in zip((24, 8, 8, 8, 8), (9, 5, 6, 3, 2))]).shape == (2, 150, 9, 9)
    # at the call: no CPU fallback; level sizes must not increase; the pyramid's rules on the last level
    from mem_amd._lib import MemhipError
    head = UPerHead(**ok)
    with pytest.raises(MemhipError) as e:
        head([torch.randn(2, 64, s, s) for s in (8, 4, 2, 2)])
    assert "UPerHead(impl='hip')" in str(e.value) and "no CPU fallback" in str(e.value)
    with pytest.raises(ValueError) as e:
        head.check(4, [(8, 8), (4, 4), (4, 5), (3, 3)], True)
    assert "level 2 of 4x5 is larger than level 1 of 4x4" in str(e.value)
    with pytest.raises(ValueError) as e:
        head.check(4, [(8, 8), (9, 4), (4, 4), (3, 3)], True)
    assert "level sizes must not increase" in str(e.value)
    head.check(4, [(8, 8), (8, 8), (6, 7), (6, 7)], True)                                  # equal sizes are allowed
    with pytest.raises(ValueError) as e:
        head.check(4, [(8, 8), (8, 8), (6, 7), (5, 7)], True)                              # pool scale 6 on 5x7
    assert "pool_scales" in str(e.value) and "5x7" in str(e.value)
    with pytest.raises(ValueError) as e:
        head.check(1, [(8, 8), (8, 8), (6, 7), (6, 7)], True)                              # B s^2 == 1 at scale 1
    assert "more than 1 value per channel" in str(e.value)
    head.check(1, [(8, 8), (8, 8), (6, 7), (6, 7)], False)
    # SegModel takes it as decode_head unchanged, and gives each head its own Dropout2d site
    from mem_amd import ops
    m = SegModel(torch.nn.Identity(), UPerHead(**ok), auxiliary_head=FCNHead(in_channels=64, channels=64, num_classes=3))
    assert (m.decode_head.dropout_site, m.auxiliary_head.dropout_site) == (ops.DROPOUT_SITE_HEAD, ops.DROPOUT_SITE_HEAD + 1)
    assert sorted(n for n in ("forward_train", "forward_test", "refresh", "reduce", "drop_key", "keep_mask") if hasattr(m.decode_head, n)) == \
        sorted(("forward_train", "forward_test", "refresh", "reduce", "drop_key", "keep_mask"))
