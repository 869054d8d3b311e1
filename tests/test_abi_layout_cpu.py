"""-m "not gpu": the ctypes mirrors of the structs in include/memhip.h, and the argument checks of the struct entry points.

Layout: a few lines of C, compiled against the header with the host compiler, print sizeof and every field's offsetof for each
`typedef struct` of the header; each is compared with the ctypes class that mirrors it (ctypes.sizeof, Class.field.offset).  The
field list comes from the header, so a mirror must name its fields as C does, in C's order.  A struct without a mirror, or a
mirror without a struct, fails.

Validation: memhip_branch_bwd, memhip_layernorm_bwd_branch, memhip_attn_bwd, memhip_conv2d_nhwc and memhip_rasterize check their
arguments before any launch, so every rule is exercised here through ctypes with dummy addresses -- nothing is dereferenced and
no case reaches a launch.  memhip_conv_plan and memhip_rasterize_plan take the struct of their call: every call that is rejected
is rejected by the query with the same code and the same message."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "memhip.h")


def _mirrors():
    from mem_amd import datasets, ops
    return {"memhip_event_aug_t": datasets.EventAug, "memhip_raster_args_t": datasets.RasterArgs,
            "memhip_raster_launch_t": datasets.RasterLaunch, "memhip_raster_plan_t": datasets.RasterPlan, "memhip_dropout_t": ops.Dropout, "memhip_gemm_args_t": ops.GemmArgs,
            "memhip_nt_launch_t": ops.NtLaunch, "memhip_nt_plan_t": ops.NtPlan,
            "memhip_tn_problem_t": ops.TnProblem, "memhip_tn_part_t": ops.TnPart, "memhip_tn_launch_t": ops.TnLaunch,
            "memhip_tn_plan_t": ops.TnPlan,
            "memhip_attn_launch_t": ops.AttnLaunch, "memhip_attn_plan_t": ops.AttnPlan,
            "memhip_conv_launch_t": ops.ConvLaunch, "memhip_conv_plan_t": ops.ConvPlan, "memhip_conv_args_t": ops.ConvArgs,
            "memhip_branch_t": ops.Branch, "memhip_branch_bwd_args_t": ops.BranchBwdArgs,
            "memhip_ln_bwd_branch_args_t": ops.LnBwdBranchArgs, "memhip_attn_bwd_args_t": ops.AttnBwdArgs}


# header structs that have no ctypes mirror, with the reason (none today)
UNMIRRORED = {}


def _header_structs():
    """{typedef name: [field names in declaration order]} of every `typedef struct` in the header"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;", src, flags=re.S):
        fields = []
        for decl in body.split(";"):
            for piece in decl.split(","):                      # `int32_t M, N, K` declares three; the name is the last identifier
                piece = re.sub(r"\[[^\]]*\]", "", piece).strip()
                if piece:
                    fields.append(re.findall(r"\w+", piece)[-1])
        out[name] = fields
    return out


def _host_cc():
    for cc in (shutil.which("cc"), "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang"):
        if cc and os.path.exists(cc):
            return cc
    return None


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    """{typedef name: (sizeof, {field: offsetof})} as the host compiler lays the header's structs out"""
    cc = _host_cc()
    if cc is None:
        pytest.skip("no host C compiler")
    structs = _header_structs()
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "memhip.h"', "int main(void) {"]
    for name, fields in structs.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f in fields]
    lines += ["  return 0;", "}"]
    tmp = tmp_path_factory.mktemp("abi_layout")
    src, exe = str(tmp / "layout.c"), str(tmp / "layout")
    open(src, "w").write("\n".join(lines) + "\n")
    r = subprocess.run([cc, "-I", os.path.dirname(HEADER), src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    layout = {name: [None, {}] for name in structs}
    printed = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    for key, value in re.findall(r"^(\S+) (\d+)$", printed, re.M):
        if "." in key:
            name, field = key.split(".")
            layout[name][1][field] = int(value)
        else:
            layout[key][0] = int(value)
    return layout


def test_every_header_struct_has_its_mirror():
    structs, mirrors = set(_header_structs()), set(_mirrors())
    assert len(structs) >= 18
    assert structs - mirrors - set(UNMIRRORED) == set(), "structs of the header without a ctypes mirror"
    assert mirrors - structs == set(), "ctypes mirrors of structs the header does not have"
    assert set(UNMIRRORED) <= structs - mirrors, "UNMIRRORED lists a struct that is gone or has a mirror"


@pytest.mark.parametrize("name", sorted(_header_structs()))
def test_mirror_layout_matches_header(c_layout, name):
    if name in UNMIRRORED:
        pytest.skip(UNMIRRORED[name])
    cls = _mirrors()[name]
    size, offsets = c_layout[name]
    assert [f[0] for f in cls._fields_] == list(offsets), (name, "field names / order differ from the header")
    assert C.sizeof(cls) == size, (name, C.sizeof(cls), size)
    for field, off in offsets.items():
        assert getattr(cls, field).offset == off, (name, field, getattr(cls, field).offset, off)


# ---------------------------------------------------------------- validation of the struct entry points, no launch
P = 0x1000          # a dummy, 16-byte aligned, non-NULL address: checked for NULL only before the launch


def _call(fn, args):
    from mem_amd import _lib
    rc = getattr(_lib.lib, fn)(None if args is None else C.byref(args), None)
    return rc, _lib.lib.memhip_last_error().decode()


def _rejected(fn, args, message):
    rc, err = _call(fn, args)
    assert rc == -1 and message in err, (fn, rc, err)


def _branch(**kw):
    from mem_amd import ops
    b = ops.Branch(y=None, ldy=0, gamma=None, rowmask=None, keep_prob=1.0, rows_per_sample=1, dy=P, lddy=8)
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def test_branch_bwd_validation():
    from mem_amd import ops
    fn = "memhip_branch_bwd"

    def args(M=4, D=8, dx=P, lddx=8, **branch):
        return ops.BranchBwdArgs(dx, lddx, M, D, _branch(**branch))
    _rejected(fn, None, "branch_bwd: null args")
    assert _call(fn, ops.BranchBwdArgs(None, 0, 0, 8, ops.Branch()))[0] == 0                   # M == 0: nothing to do
    _rejected(fn, args(D=6), "branch_bwd: bad M=4 D=6")
    drop = ops.dropout_params(1, 2, 0, 0.1)
    _rejected(fn, args(D=4, lddx=4, lddy=4, dropout=C.addressof(drop)), "D=4 must be a multiple of 8")
    _rejected(fn, args(out_map=P, rowmask=P), "branch_bwd: out_map excludes rowmask / y")
    _rejected(fn, args(out_map=P, y=P, ldy=8), "branch_bwd: out_map excludes rowmask / y")
    _rejected(fn, args(dx=None), "branch_bwd: null pointer")
    _rejected(fn, args(dy=None), "branch_bwd: null pointer")
    _rejected(fn, args(dgamma=P), "branch_bwd: dgamma needs y")
    _rejected(fn, args(lddx=6), "branch_bwd: ld must be a multiple of 4")
    _rejected(fn, args(lddy=10), "branch_bwd: ld must be a multiple of 4")
    _rejected(fn, args(y=P, ldy=2), "branch_bwd: ld must be a multiple of 4")
    _rejected(fn, args(D=2052, lddx=2052, lddy=2052), "branch_bwd: D=2052 too large")


def test_layernorm_bwd_branch_validation():
    from mem_amd import ops
    fn = "memhip_layernorm_bwd_branch"

    def args(R=4, D=8, in_map=None, **kw):
        a = ops.LnBwdBranchArgs(P, 8, P, 8, R, D, P, P, P, P, 8, P, P, in_map, _branch())
        for k, v in kw.items():
            setattr(a.branch if k.startswith("b_") else a, k[2:] if k.startswith("b_") else k, v)
        return a
    _rejected(fn, None, "layernorm_bwd_branch: null args")
    assert _call(fn, ops.LnBwdBranchArgs(R=0, D=8))[0] == 0                                    # R == 0: nothing to do
    _rejected(fn, args(D=1028), "layernorm_bwd_branch: D=1028 unsupported (<= 1024)")
    drop = ops.dropout_params(1, 2, 0, 0.1)
    _rejected(fn, args(D=4, b_dropout=C.addressof(drop)), "D=4 must be a multiple of 8")
    _rejected(fn, args(in_map=P, b_rowmask=P), "layernorm_bwd_branch: sample maps exclude rowmask / y_branch")
    _rejected(fn, args(b_out_map=P, b_y=P), "layernorm_bwd_branch: sample maps exclude rowmask / y_branch")
    for field in ("dy", "x", "gamma", "mean", "rstd", "dres", "dgamma", "dbeta", "b_dy"):
        _rejected(fn, args(**{field: None}), "layernorm_bwd_branch: null pointer")
    _rejected(fn, args(b_dgamma=P), "layernorm_bwd_branch: dgamma_branch needs y_branch")
    for field in ("ldx", "lddy", "lddres", "b_ldy", "b_lddy"):
        _rejected(fn, args(**{field: 6}), "layernorm_bwd_branch: ld must be a multiple of 4")


def test_attn_bwd_validation():
    from mem_amd import ops
    fn = "memhip_attn_bwd"

    def args(B=2, T=197, D=768, heads=12, window=(14, 14), **kw):
        a = ops.AttnBwdArgs(P, 3 * D, P, D, None, 0, P, P, P, window[0], window[1], B, T, D, heads, 0.125, 0, P, 3 * D, P, None,
                            None, None, 0)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    _rejected(fn, None, "attn_bwd: null args")
    assert _call(fn, ops.AttnBwdArgs(window_h=14, window_w=14, B=0, T=197, D=768, heads=12))[0] == 0   # B == 0: nothing to do
    _rejected(fn, args(D=760), "attn_bwd: head_dim must be 64")
    _rejected(fn, args(T=196), "attn_bwd: T must be window_h*window_w + 1")
    _rejected(fn, args(window=(14, 0)), "attn_bwd: T must be window_h*window_w + 1")
    for field in ("qkv", "dout", "lse", "delta", "table", "dqkv"):
        _rejected(fn, args(**{field: None}), "attn_bwd: null pointer")
    for field in ("ldqkv", "ldo", "ldout", "lddqkv"):
        _rejected(fn, args(**{field: 772}), "attn_bwd: ld must be a multiple of 8")


def test_conv2d_nhwc_validation_and_the_plan_query_agree():
    """Every rejection rule of the three modes, the rejections of a field the mode does not have, the empty batch and
    args == NULL -- and for each rejected struct memhip_conv_plan answers with the same code and the same message."""
    from mem_amd import _lib, ops
    fn = "memhip_conv2d_nhwc"
    BF16, F32, F16X2 = range(3)

    def args(mode, B=2, H=14, W=14, Cin=64, Cout=64, k=3, s=1, p=1, **kw):
        a = ops.conv_args(mode, B, H, W, Cin, Cout, k, s, p, x=P, weight=P, out=P)
        for key, v in kw.items():
            setattr(a, key, v)
        return a

    def rejected(a, message):
        """by the call and by the query alike"""
        rc, err = _call(fn, a)
        assert rc == -1 and message in err, (rc, err)
        plan = ops.ConvPlan()
        rc_q = _lib.lib.memhip_conv_plan(None if a is None else C.byref(a), 256, C.byref(plan))
        assert (rc_q, _lib.lib.memhip_last_error().decode()) == (rc, err)

    rejected(None, "conv2d: null args")
    rejected(args(3), "conv2d: unknown mode 3")
    rejected(args(-1), "conv2d: unknown mode -1")
    # a field that the mode does not have
    for mode in (BF16, F16X2):
        rejected(args(mode, n_active=P), "conv2d: only the fp32 mode has a dynamic batch (n_active)")
    for mode in (BF16, F32):
        rejected(args(mode, out_f32=1, out_padded=0), "conv2d: out_f32 is a flag of the fp16x2 mode")
        for plane in ("in_plane", "w_plane", "add_plane", "out_plane"):
            rejected(args(mode, **{plane: 4096}), "conv2d: plane strides are fields of the fp16x2 mode")
    # the two 16-bit modes, each under its own name
    for mode, name in ((BF16, "conv2d"), (F16X2, "conv2d_f16x2")):
        for bad in (dict(B=-1), dict(H=0), dict(W=-3), dict(Cin=0), dict(Cout=0)):
            rejected(args(mode, **bad), name + ": bad shape")
        for k, s, p in ((2, 2, 0), (4, 1, 1), (3, 1, 0), (1, 1, 1), (3, 2, 1), (5, 1, 1)):
            rejected(args(mode, k=k, s=s, p=p), name + ": only the encoder's shapes (4x4/s2/p1, 3x3/s1/p1, 1x1) are provided")
        rejected(args(mode, Cin=32), name + ": C_in must be 4 (first layer, 4x4) or a multiple of 64")
        rejected(args(mode, Cin=4), name + ": C_in must be 4 (first layer, 4x4) or a multiple of 64")       # 3x3 on 4 channels
        rejected(args(mode, Cout=36), name + ": C_out must be a multiple of 8")
        rejected(args(mode, B=1 << 20, H=224, W=224, k=1, s=1, p=0), name + ": too many output pixels")
    rejected(args(F16X2, out_f32=1, out_padded=1), "conv2d_f16x2: the fp32 output is the dense token-logit matrix")
    # the fp32 mode
    for bad in (dict(B=-1), dict(H=0), dict(W=-3), dict(Cin=0), dict(Cout=0)):
        rejected(args(F32, **bad), "conv2d_f32: bad shape")
    for k, s, p in ((0, 1, 1), (5, 1, 1), (3, 0, 1), (3, 1, -1), (3, 1, 2)):
        rejected(args(F32, k=k, s=s, p=p), "conv2d_f32: kernel size 1..4, padding 0 or 1 (one-pixel border layout)")
    rejected(args(F32, Cin=6), "conv2d_f32: C_in and C_out must be multiples of 4")
    rejected(args(F32, Cout=10), "conv2d_f32: C_in and C_out must be multiples of 4")
    rejected(args(F32, H=2, W=2, k=4, p=0), "conv2d_f32: empty output")
    rejected(args(F32, Cin=4), "conv2d_f32: K = 36 must be a multiple of 32")
    rejected(args(F32, B=1 << 20, H=224, W=224, k=1, s=1, p=0), "conv2d_f32: too many output pixels")
    for mode, name in ((BF16, "conv2d"), (F32, "conv2d_f32"), (F16X2, "conv2d_f16x2")):
        # the call alone needs in / weight / out; the query asks about a call it does not make
        for field in ("in", "weight", "out"):
            _rejected(fn, args(mode, **{field: None}), name + ": null pointer")
        # an empty batch: nothing to do, nothing read
        assert _call(fn, ops.conv_args(mode, 0, 14, 14, 64, 64, 3, 1, 1))[0] == 0


def test_rasterize_validation_and_the_plan_query_agree():
    """Every rejection rule of memhip_rasterize, the empty batch and args == NULL -- and for each rejected struct
    memhip_rasterize_plan answers with the same code and the same message."""
    from mem_amd import _lib, datasets as D
    fn = "memhip_rasterize"

    def args(B=2, H=224, W=224, ts=False, form=D.RASTER_AUTO, n_events=1000, **kw):
        a = D.raster_args(B, H, W, ts, form, n_events, ev=P, offsets=P, out=P, status=P, workspace=P, workspace_bytes=1 << 40)
        for key, v in kw.items():
            setattr(a, key, v)
        return a

    def rejected(a, message, code=-1):
        """by the call and by the query alike"""
        rc, err = _call(fn, a)
        assert rc == code and message in err, (rc, err)
        plan = D.RasterPlan()
        rc_q = _lib.lib.memhip_rasterize_plan(None if a is None else C.byref(a), 256, C.byref(plan))
        assert (rc_q, _lib.lib.memhip_last_error().decode()) == (rc, err)

    rejected(None, "rasterize: null args")
    for bad in (dict(B=-1), dict(H=0), dict(W=-3)):
        rejected(args(**bad), "rasterize: bad shape B=%d H=%d W=%d" % tuple(dict(dict(B=2, H=224, W=224), **bad).values()))
    rejected(args(n_events=-1), "rasterize: n_events=-1 must not be negative")
    for form in (-1, 3, D.RASTER_LDS):
        rejected(args(form=form), "rasterize: unknown form %d" % form)
    rejected(args(ts=True, form=D.RASTER_BINNED), "rasterize: the binned form has no time surface and no per-sample canvases")
    rejected(args(dims=P, form=D.RASTER_BINNED), "rasterize: the binned form has no time surface and no per-sample canvases")
    rejected(args(B=0, dims=P, form=D.RASTER_BINNED), "rasterize: the binned form has no time surface and no per-sample canvases")
    for form in (D.RASTER_AUTO, D.RASTER_SINGLE, D.RASTER_BINNED):
        rejected(args(form=form, ev=P + 8), "rasterize: ev must be 16-byte aligned")
    # the two-pass kernels store 4 bytes at a time; AUTO chooses them for this canvas, the single-pass forms take any `out`
    for form in (D.RASTER_AUTO, D.RASTER_BINNED):
        rejected(args(form=form, out=P + 2), "rasterize: out must be 4-byte aligned for the binned form")
    rejected(args(H=1601, W=1600, form=D.RASTER_BINNED), "rasterize: 1601x1600 canvas needs more than 64 bands", code=-4)
    # workspace too small, per family: the query compares workspace_bytes whenever it is given a workspace
    for kw in (dict(form=D.RASTER_BINNED), dict(form=D.RASTER_SINGLE), dict(form=D.RASTER_SINGLE, ts=True), dict(dims=P)):
        need = D.raster_plan(args(workspace=None, **kw), 256).ws_bytes
        assert need > 0
        rejected(args(workspace_bytes=need - 1, **kw), "rasterize: workspace %d < %d" % (need - 1, need), code=-2)
    # the call alone needs its pointers; the query asks about a call it does not make
    for field in ("ev", "offsets", "out", "status", "workspace"):
        _rejected(fn, args(**{field: None}), "rasterize: null pointer")
        assert _lib.lib.memhip_rasterize_plan(C.byref(args(**{field: None})), 256, C.byref(D.RasterPlan())) == 0
    # an empty batch: nothing to do, nothing read
    assert _call(fn, D.raster_args(0, 224, 224))[0] == 0
