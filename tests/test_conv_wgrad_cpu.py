"""-m "not gpu": the host side of the convolution weight gradient (csrc/conv_wgrad.hip, conv_wgrad_plan.{hpp,cpp}) and of the
data-gradient weight packers (mem_amd/vae_model.py dgrad_weight / pack_dgrad_weight).

memhip_conv_wgrad_plan validates like the call and describes the launch without a device; the gather arithmetic the kernel
shares with the host (wgrad_gather) is enumerated by a stand-alone program (tests/wgrad_addr_check.cpp, built here with the
host sanitizers) for every shape the GPU tests run; the packers are checked against autograd in float64 on non-square shapes."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

P = 0x1000                                                  # a dummy, 16-byte aligned, non-NULL address

# (ksize, stride, pad, B, Hs, Ws, C, N, small_padded): Hs x Ws is the SMALL grid, big is [B, s*Hs+2, s*Ws+2, C].  H != W everywhere.
SHAPES = {
    "4x4s2_one_tile_ragged_n": (4, 2, 1, 3, 5, 7, 128, 72, 1),       # M = 105 < one stage pair, N ragged in the tile
    "4x4s2_first_layer_c4": (4, 2, 1, 2, 6, 10, 4, 64, 1),
    "3x3_tile_spans_two_taps": (3, 1, 1, 3, 5, 7, 64, 136, 1),
    "3x3_tile_straddles_a_tap": (3, 1, 1, 2, 5, 7, 192, 64, 1),
    "1x1_padded_small_n8": (1, 1, 0, 3, 5, 7, 128, 8, 1),
    "1x1_dense_small": (1, 1, 0, 3, 5, 7, 64, 264, 0),
    "transposed_roles": (4, 2, 1, 3, 5, 7, 72, 128, 1),               # small = the layer's input (128), big = g of the output (72)
    "3x3_many_slices": (3, 1, 1, 4, 28, 28, 64, 64, 1),               # M = 3136 = 49 stages: 10 slices of 5
    "4x4s2_three_slices": (4, 2, 1, 4, 14, 14, 64, 64, 1),            # big [4, 30, 30, 64]; M = 784: 3 slices
}


def base_vae_layers(B=32):
    """Every conv_wgrad call of one training step of the ViT-B tokenizer (oracle.vae_ref.BASE_VAE)."""
    from oracle.vae_ref import BASE_VAE as V
    hid, L = V["hidden_dim"], V["num_layers"]
    out = []
    h, w = V["input_H"], V["input_W"]
    for i in range(L):                                       # encoder Conv2d(4, 2, 1); decoder ConvTranspose2d (roles swapped)
        h, w = h // 2, w // 2
        out.append((4, 2, 1, B, h, w, 4 if i == 0 else hid, hid, 1))
        out.append((4, 2, 1, B, h, w, hid, hid, 1))
    out += [(3, 1, 1, B, h, w, hid, hid, 1), (1, 1, 0, B, h, w, hid, hid, 1)]            # the ResBlocks
    out.append((1, 1, 0, B, h, w, hid, V["num_tokens"], 0))                              # token logits: dense small
    out.append((1, 1, 0, B, h, w, V["codebook_dim"], hid, 1))                            # the 1x1 behind the codebook
    out.append((1, 1, 0, B, V["input_H"], V["input_W"], hid, 8, 0))                      # reconstruction head: dense, 8 channels
    return list(dict.fromkeys(out))


def _err():
    from mem_amd import _lib
    return _lib.lib.memhip_last_error().decode()


def test_symbols_exported_and_abi_unchanged():
    from mem_amd import _lib
    for name in ("memhip_conv_wgrad_nhwc", "memhip_conv_wgrad_plan", "memhip_conv_wgrad_workspace", "memhip_relu_bwd_colsum",
                 "memhip_relu_bwd_colsum_workspace"):
        assert hasattr(_lib.lib, name), name
    assert _lib.lib.memhip_abi_version() == 10


def test_struct_mirrors_match_the_header(tmp_path):
    """sizeof and every offsetof of the two structs, as the host compiler lays them out, against the ctypes mirrors."""
    from mem_amd import ops
    cc = next((c for c in (shutil.which("cc"), "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang") if c and os.path.exists(c)), None)
    if cc is None:
        pytest.skip("no host C compiler")
    header = open(os.path.join(ROOT, "include", "memhip.h")).read()
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "memhip.h"', "int main(void) {"]
    mirrors = {"memhip_conv_wgrad_args": ops.ConvWgradArgs, "memhip_conv_wgrad_plan": ops.ConvWgradPlan}
    for tag, cls in mirrors.items():
        body = re.search(r"struct\s+%s\s*\{(.*?)\};" % tag, re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S).group(1)
        fields = [re.findall(r"\w+", piece)[-1] for decl in body.split(";") for piece in decl.split(",") if piece.strip()]
        assert fields == [f[0] for f in cls._fields_], (tag, fields)
        lines.append('  printf("%s %%zu\\n", sizeof(struct %s));' % (tag, tag))
        lines += ['  printf("%s.%s %%zu\\n", offsetof(struct %s, %s));' % (tag, f, tag, f) for f in fields]
    lines += ["  return 0;", "}"]
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    open(src, "w").write("\n".join(lines) + "\n")
    r = subprocess.run([cc, "-I", os.path.join(ROOT, "include"), src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    printed = dict(re.findall(r"^(\S+) (\d+)$", subprocess.run([exe], capture_output=True, text=True, check=True).stdout, re.M))
    for tag, cls in mirrors.items():
        assert C.sizeof(cls) == int(printed[tag]), tag
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == int(printed[tag + "." + f]), (tag, f)


def test_validation_and_the_plan_query_agree():
    from mem_amd import _lib, ops
    lib = _lib.lib

    def args(k=3, s=1, p=1, B=2, Hs=5, Ws=7, C_=64, N=64, **kw):
        a = ops.conv_wgrad_args(B, Hs, Ws, C_, N, k, s, p, small=P, big=P, grad=P, workspace=P, workspace_bytes=1 << 40)
        for key, v in kw.items():
            setattr(a, key, v)
        return a

    def rejected(a, message):
        rc = lib.memhip_conv_wgrad_nhwc(None if a is None else C.byref(a), None)
        err = _err()
        assert rc == -1 and message in err, (rc, err)
        rc_q = lib.memhip_conv_wgrad_plan(None if a is None else C.byref(a), 256, C.byref(ops.ConvWgradPlan()))
        assert (rc_q, _err()) == (rc, err)
        assert lib.memhip_conv_wgrad_workspace(None if a is None else C.byref(a), 256) == 0

    rejected(None, "conv_wgrad: null args")
    for bad in (dict(B=-1), dict(Hs=0), dict(Ws=-3), dict(C_=0), dict(N=0)):
        rejected(args(**bad), "conv_wgrad: bad shape")
    for k, s, p in ((2, 2, 0), (4, 1, 1), (3, 1, 0), (1, 1, 1), (3, 2, 1), (5, 1, 1), (4, 2, 0)):
        rejected(args(k=k, s=s, p=p), "conv_wgrad: only the forms (4, 2, 1), (3, 1, 1), (1, 1, 0) are provided, got (%d, %d, %d)" % (k, s, p))
    rejected(args(C_=4), "conv_wgrad: C must be 4 (first layer, 4x4) or a multiple of 8, got 4")          # 3x3 on 4 channels
    rejected(args(C_=12), "conv_wgrad: C must be 4 (first layer, 4x4) or a multiple of 8, got 12")
    rejected(args(N=36), "conv_wgrad: N must be a multiple of 8, got 36")
    rejected(args(small_padded=2), "conv_wgrad: small_padded is 0 or 1")
    rejected(args(accumulate=-1), "conv_wgrad: accumulate is 0 or 1")
    rejected(args(k=1, s=1, p=0, B=1 << 12, Hs=1 << 10, Ws=1 << 10), "conv_wgrad: too many pixels or channels")
    # the call alone needs its pointers and their alignment; the query asks about a call it does not make
    for field in ("small", "big", "grad"):
        a = args(**{field: None})
        assert lib.memhip_conv_wgrad_nhwc(C.byref(a), None) == -1 and "conv_wgrad: null pointer" in _err()
        assert lib.memhip_conv_wgrad_plan(C.byref(a), 256, C.byref(ops.ConvWgradPlan())) == 0
    for field in ("small", "big"):
        a = args(**{field: P + 8})
        assert lib.memhip_conv_wgrad_nhwc(C.byref(a), None) == -1 and "16-byte aligned" in _err()
    a = args()
    assert lib.memhip_conv_wgrad_plan(C.byref(a), 256, None) == -1 and "conv_wgrad_plan: null pointer" in _err()
    # an empty batch: nothing to do, nothing read
    e = ops.conv_wgrad_args(0, 5, 7, 64, 64, 3, 1, 1)
    assert lib.memhip_conv_wgrad_nhwc(C.byref(e), None) == 0
    p = ops.conv_wgrad_plan(0, 5, 7, 64, 64, 3, 1, 1, device_cus=256)
    assert (p.M, p.grid, p.splits, p.ws_bytes) == (0, 0, 0, 0)
    # relu_bwd_colsum
    for bad in (dict(B=-1), dict(H=0), dict(W=0), dict(C_=12), dict(C_=0)):
        kw = dict(dict(B=2, H=5, W=7, C_=64), **bad)
        rc = lib.memhip_relu_bwd_colsum(P, P, 1, kw["B"], kw["H"], kw["W"], kw["C_"], None, 0, None, 0, None)
        assert rc == -1 and "relu_bwd_colsum: bad shape" in _err(), bad
    assert lib.memhip_relu_bwd_colsum(None, P, 1, 2, 5, 7, 64, None, 0, None, 0, None) == -1 and "null pointer" in _err()
    assert lib.memhip_relu_bwd_colsum(P, P, 1, 2, 5, 7, 64, P, 0, None, 0, None) == -1 and "need a workspace" in _err()
    assert lib.memhip_relu_bwd_colsum(P, P, 1, 2, 5, 7, 64, P, 0, P, 8, None) == -2 and "workspace 8 <" in _err()
    assert lib.memhip_relu_bwd_colsum(None, None, 1, 0, 5, 7, 64, None, 0, None, 0, None) == 0
    assert ops.relu_bwd_colsum_workspace(2, 5, 7, 64) == 2 * 64 * 4              # 70 rows: two blocks of 64


@pytest.mark.parametrize("shape", list(SHAPES.values()) + base_vae_layers(), ids=lambda s: "x".join(map(str, s)))
def test_plan_properties(shape):
    """grid = tiles x slices; the slices cover [0, M) once in whole 64-row stages and none is empty; the workspace bytes are
    what the launches write (one [N, K] fp32 slab per slice, none with one slice); LDS <= 160 KiB."""
    from mem_amd import ops
    k, s, pad, B, Hs, Ws, C_, N, padded = shape
    p = ops.conv_wgrad_plan(B, Hs, Ws, C_, N, k, s, pad, small_padded=bool(padded), device_cus=256)
    M, K = B * Hs * Ws, k * k * C_
    assert (p.M, p.K, p.Hbp, p.Wbp) == (M, K, s * Hs + 2, s * Ws + 2)
    assert (p.tiles_n, p.tiles_k) == (-(-N // 128), -(-K // 128))
    assert p.grid == p.tiles_n * p.tiles_k * p.splits and p.block == 256 and 0 < p.lds_bytes <= 160 * 1024
    assert p.splits >= 1 and p.rows_per_split % 64 == 0
    covered = [(i * p.rows_per_split, min(M, (i + 1) * p.rows_per_split)) for i in range(p.splits)]
    assert covered[0][0] == 0 and covered[-1][1] == M and all(a < b for a, b in covered)
    assert all(covered[i][1] == covered[i + 1][0] for i in range(p.splits - 1))
    assert p.ws_bytes == (p.splits * N * K * 4 if p.splits > 1 else 0)
    assert p.fold_grid == (-(-N * K // 256) if p.splits > 1 else 0)
    assert ops.conv_wgrad_workspace(B, Hs, Ws, C_, N, k, s, pad, small_padded=bool(padded), device_cus=256) == p.ws_bytes
    # where the reduction is long enough to cut, the slices fill the 512 workgroup slots of 256 CUs once: never a second round,
    # and less than one more slice per tile would fit
    if M >= 64 * 4 * 512:
        tiles = p.tiles_n * p.tiles_k
        assert 512 - tiles < p.grid <= 512 or tiles > 512


def test_plan_slices_at_the_shapes_of_the_gpu_tests():
    from mem_amd import ops
    got = {name: ops.conv_wgrad_plan(B, Hs, Ws, C_, N, k, s, pad, small_padded=bool(pd), device_cus=256).splits
           for name, (k, s, pad, B, Hs, Ws, C_, N, pd) in SHAPES.items()}
    assert got["4x4s2_one_tile_ragged_n"] == 1 and got["3x3_many_slices"] == 10 and got["4x4s2_three_slices"] == 3, got


def test_address_function_program(tmp_path):
    """tests/wgrad_addr_check.cpp with the host sanitizers: every address wgrad_gather can give the kernel, for every shape of
    the GPU tests, lies inside its buffer and equals the brute-force definition."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "wgrad_addr_check")
    base = [hipcc, "-O1", "-g", "-std=c++17", "--cuda-host-only", os.path.join(ROOT, "tests", "wgrad_addr_check.cpp"), "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    sanitized = r.returncode == 0
    if not sanitized:
        # only a toolchain WITHOUT the sanitizer runtimes may fall back to the asserts alone; any other failure of the
        # sanitizer build (a compile error that shows only under -fsanitize) fails here
        assert re.search(r"clang_rt|libclang_rt|sanitizer runtime|cannot find -l|unsupported option '-fsanitize", r.stderr), r.stderr[-3000:]
        r = subprocess.run(base, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    print("wgrad_addr_check built %s" % ("with -fsanitize=address,undefined" if sanitized else "WITHOUT sanitizers (runtimes not installed)"))
    specs = [",".join(map(str, s)) for s in SHAPES.values()]
    r = subprocess.run([exe] + specs, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.count("ok ") == len(specs)


# ---------------------------------------------------------------- the data-gradient weights (vae_model.dgrad_weight)
def _autograd_dx(fn, x):
    x = x.clone().requires_grad_(True)
    y = fn(x)
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    (y * g).sum().backward()
    return g, x.grad


@pytest.mark.parametrize("kind", ["conv4s2", "convt", "conv3", "conv1"])
def test_dgrad_weights_vs_autograd(kind):
    """F.conv2d / F.conv_transpose2d of g with the re-read weight == autograd's input gradient, float64, H != W, Cin != Cout."""
    from mem_amd.vae_model import dgrad_weight
    gen = torch.Generator().manual_seed(3)
    B, H, W, ci, co = 2, 6, 10, 5, 3
    x = torch.randn(B, ci, H, W, generator=gen, dtype=torch.float64)
    if kind == "convt":
        w = torch.randn(ci, co, 4, 4, generator=gen, dtype=torch.float64)
        fwd = lambda t: F.conv_transpose2d(t, w, stride=2, padding=1)
    else:
        k, s, p = {"conv4s2": (4, 2, 1), "conv3": (3, 1, 1), "conv1": (1, 1, 0)}[kind]
        w = torch.randn(co, ci, k, k, generator=gen, dtype=torch.float64)
        fwd = lambda t: F.conv2d(t, w, stride=s, padding=p)
    g, want = _autograd_dx(fwd, x)
    op, wd = dgrad_weight(kind, w)
    if op == "conv_transpose2d":
        got = F.conv_transpose2d(g, wd, stride=2, padding=1)
    else:
        got = F.conv2d(g, wd, stride=2 if kind == "convt" else 1, padding=1 if kind in ("convt", "conv3") else 0)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= 1e-12


@pytest.mark.parametrize("kind", ["conv4s2", "convt", "conv3", "conv1"])
def test_packed_dgrad_weights_are_the_kernels_layouts(kind):
    """pack_dgrad_weight = the forward kernels' own packers applied to dgrad_weight, zero padding included."""
    from mem_amd.vae_model import dgrad_weight, pack_conv_weight, pack_convt_weight, pack_dgrad_weight
    gen = torch.Generator().manual_seed(5)
    k = {"conv4s2": 4, "convt": 4, "conv3": 3, "conv1": 1}[kind]
    w = torch.randn(3, 5, k, k, generator=gen, dtype=torch.float64)
    op, wd = dgrad_weight(kind, w)
    want = pack_convt_weight(wd) if op == "conv_transpose2d" else pack_conv_weight(wd)
    assert torch.equal(pack_dgrad_weight(kind, w), want)
    assert pack_conv_weight(w).shape == (3, k * k * 5) and torch.equal(pack_conv_weight(w).view(3, k, k, 5)[1, k - 1, 0], w[1, :, k - 1, 0])
    if op == "conv2d":
        co, ci = wd.shape[:2]
        pp = pack_dgrad_weight(kind, w, cin_pad=ci + 3, cout_pad=co + 1).view(co + 1, k, k, ci + 3)
        assert torch.equal(pp[:co, :, :, :ci].reshape(co, -1), want) and pp[co:].abs().max() == 0 and pp[..., ci:].abs().max() == 0
