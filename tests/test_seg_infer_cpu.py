"""-m "not gpu": the host side of segmentation inference: the sliding-window grid, the layout of the two structs of
memhip_seg_predict, every validation rule of the call and of its plan query (dummy addresses, nothing is dereferenced, no case
reaches a launch), the inference tool's flags and refusals, the palette and the painter."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "memhip.h")
P = 0x1000          # a dummy, 16-byte aligned, non-NULL address


# ---------------------------------------------------------------- slide_windows
def _counts(canvas, crop, wins):
    cnt = np.zeros(canvas, dtype=np.int64)
    for y1, x1 in wins:
        assert 0 <= y1 and y1 + crop[0] <= canvas[0] and 0 <= x1 and x1 + crop[1] <= canvas[1], (y1, x1)
        cnt[y1:y1 + crop[0], x1:x1 + crop[1]] += 1
    return cnt


def test_slide_windows_worked_cases():
    from mem_amd.seg_infer import slide_windows
    wins = slide_windows((48, 64), (32, 32), (16, 24))
    assert wins == [(0, 0), (0, 24), (0, 32), (16, 0), (16, 24), (16, 32)]
    cnt = _counts((48, 64), (32, 32), wins)
    assert cnt.min() >= 1 and set(np.unique(cnt)) == {1, 2, 4}
    wins = slide_windows((45, 70), (32, 40), (21, 27))
    assert wins == [(0, 0), (0, 27), (0, 30), (13, 0), (13, 27), (13, 30)]
    cnt = _counts((45, 70), (32, 40), wins)
    assert cnt.min() >= 1 and set(np.unique(cnt)) == {1, 2, 3, 4, 6}
    assert slide_windows((48, 64), (48, 64), (16, 16)) == [(0, 0)]
    assert slide_windows((440, 640), (256, 256), (171, 171)) == [(y, x) for y in (0, 171, 184) for x in (0, 171, 342, 384)]
    for canvas, crop, stride in (((440, 640), (256, 256), (171, 171)), ((37, 53), (16, 20), (11, 7)), ((33, 33), (32, 32), (32, 32))):
        assert _counts(canvas, crop, slide_windows(canvas, crop, stride)).min() >= 1       # covered, and inside (in _counts)
    with pytest.raises(ValueError, match="positive"):
        slide_windows((48, 64), (32, 32), (0, 8))


# ---------------------------------------------------------------- layout of the two structs
def _host_cc():
    for cc in (shutil.which("cc"), "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang"):
        if cc and os.path.exists(cc):
            return cc
    return None


def test_struct_layout_matches_header(tmp_path):
    from mem_amd import ops
    cc = _host_cc()
    if cc is None:
        pytest.skip("no host C compiler")
    mirrors = {"memhip_segpredict_args_t": ops.SegPredictArgs, "memhip_segpredict_plan_t": ops.SegPredictPlan}
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "memhip.h"', "int main(void) {"]
    for name, cls in mirrors.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f[0], name, f[0]) for f in cls._fields_]
    lines += ["  return 0;", "}"]
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    open(src, "w").write("\n".join(lines) + "\n")
    r = subprocess.run([cc, "-I", os.path.dirname(HEADER), src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]                 # a mirror's field that the header lacks does not compile
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for name, cls in mirrors.items():
        assert C.sizeof(cls) == int(got[name]), (name, C.sizeof(cls), got[name])
        covered = 0
        for field, ctype in cls._fields_:
            assert getattr(cls, field).offset == int(got["%s.%s" % (name, field)]), (name, field)
            covered += C.sizeof(ctype)
        assert covered == C.sizeof(cls), (name, "padding or a field of the header without a mirror")


# ---------------------------------------------------------------- validation, call and plan query alike
GRID = [(0, 0, 0), (0, 24, 0), (0, 32, 0), (16, 0, 0), (16, 24, 0), (16, 32, 0)]      # 32 x 32 windows on 48 x 64


def _args(rects=GRID, B=2, C_=5, hw=(8, 8), window=(32, 32), out_size=(48, 64), **fields):
    from mem_amd import ops
    f = dict(logits=P, y_i0=P, y_w1=P, x_i0=P, x_w1=P, pred=P)
    f.update(fields)
    return ops.seg_predict_args(rects, B, C_, hw, window, out_size, **f)


def _both(a):
    """(rc, message) of the call and of the plan query"""
    from mem_amd import _lib, ops
    rc = _lib.lib.memhip_seg_predict(C.byref(a), None)
    msg = _lib.lib.memhip_last_error().decode()
    plan = ops.SegPredictPlan()
    rc2 = _lib.lib.memhip_seg_predict_plan(C.byref(a), C.byref(plan))
    return (rc, msg), (rc2, _lib.lib.memhip_last_error().decode())


BAD = {
    "V=0": (dict(rects=[]), "V=0"),
    "V=65": (dict(rects=[(0, 0, 0)] * 65), "V=65"),
    "C=1": (dict(C_=1), "C=1"),
    "C=33": (dict(C_=33), "C=33"),
    "hc<h": (dict(hw=(33, 8)), "hc >= h"),
    "wc<w": (dict(hw=(8, 33)), "wc >= w"),
    "h=0": (dict(hw=(0, 8)), "h >= 1"),
    "hc>H": (dict(out_size=(31, 64), rects=[(0, 0, 0)]), "hc <= H"),
    "wc>W": (dict(out_size=(48, 31), rects=[(0, 0, 0)]), "wc <= W"),
    "rect below": (dict(rects=GRID[:5] + [(17, 32, 0)]), "leaves the canvas"),
    "rect right": (dict(rects=GRID[:5] + [(16, 33, 0)]), "leaves the canvas"),
    "rect negative": (dict(rects=GRID[:5] + [(-1, 32, 0)]), "leaves the canvas"),
    "flip=2": (dict(rects=GRID[:5] + [(16, 32, 2)]), "flip=2"),
    "uncovered": (dict(rects=GRID[:5]), "covered by no view"),
    "flipped pass uncovered": (dict(rects=GRID + [(0, 0, 1)]), "flip=1 is covered by no view"),
    "labels without confusion": (dict(labels=P), "labels and confusion"),
    "confusion without labels": (dict(confusion=P), "labels and confusion"),
    "no output": (dict(pred=None), "no output"),
    "align_corners=2": (dict(align_corners=2), "align_corners=2"),
    "B<0": (dict(B=-1), "B=-1"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_every_rule_rejects_before_any_launch_and_the_plan_agrees(case):
    kw, needle = BAD[case]
    a, keep = _args(**kw)
    (rc, msg), (rc2, msg2) = _both(a)
    assert rc == -1 and needle in msg, (case, rc, msg)
    assert (rc2, msg2) == (rc, msg), (case, msg, msg2)


def test_null_device_pointers_are_the_calls_business_only():
    from mem_amd import _lib
    for kw in (dict(logits=None), dict(x_w1=None)):
        a, keep = _args(**kw)
        (rc, msg), (rc2, _) = _both(a)
        assert rc == -1 and "null pointer" in msg and rc2 == 0
    a, keep = _args()
    a.rects = None
    (rc, msg), (rc2, msg2) = _both(a)
    assert rc == rc2 == -1 and "rects" in msg and msg2 == msg
    assert _lib.lib.memhip_seg_predict(None, None) == -1


def test_empty_batch_is_ok_and_reads_nothing():
    a, keep = _args(B=0, rects=[], C_=1, pred=None, logits=None)          # nothing else is looked at
    (rc, _), (rc2, _) = _both(a)
    assert rc == 0 and rc2 == 0


def test_plan_query_as_data():
    from mem_amd import ops
    plan = ops.seg_predict_plan(GRID, 2, 11, (8, 8), (32, 32), (48, 64), pred=P)
    assert (plan.tile_h, plan.tile_w, plan.tiles_y, plan.tiles_x) == (16, 64, 3, 1) and plan.grid == 6 and plan.block == 256
    assert plan.pixels_per_thread * (plan.block // plan.tile_h) == plan.tile_w
    assert plan.lds_bytes == 32 * 32 * 4 and plan.padded_classes == 12 and plan.passes == 1 and plan.max_count == 4
    assert plan.pred_dwords == 1
    both = GRID + [(y, x, 1) for y, x, _ in GRID]
    plan = ops.seg_predict_plan(both, 3, 19, (8, 10), (32, 32), (48, 64), prob=P)
    assert plan.passes == 2 and plan.max_count == 4 and plan.padded_classes == 20 and plan.grid == 9 and plan.pred_dwords == 0
    assert ops.seg_predict_plan([(0, 0, 1)], 1, 2, (12, 16), (45, 70), (45, 70), pred=P + 1).passes == 1
    plan = ops.seg_predict_plan([(0, 0, 0)], 1, 32, (12, 16), (45, 70), (45, 70), pred=P)
    assert (plan.tiles_y, plan.tiles_x, plan.max_count, plan.padded_classes, plan.pred_dwords) == (3, 2, 1, 32, 0)      # 70 % 4 != 0
    assert ops.seg_predict_plan([(0, 0, 0)], 1, 8, (12, 16), (48, 64), (48, 64), pred=P + 1).pred_dwords == 0           # unaligned
    # 64 thin windows: every column band once, except where the last is pulled back
    thin = [(0, min(x, 126), 0) for x in range(0, 128, 2)]
    assert ops.seg_predict_plan(thin, 1, 4, (4, 2), (8, 2), (8, 128), pred=P).max_count == 1


# ---------------------------------------------------------------- the tool
CKPT = ["--checkpoint", "x.pth"]


def test_tool_flag_defaults():
    from mem_amd import infer_semseg as T, run_semseg as R
    a = T.get_args(CKPT + ["--eval"])
    assert (a.split, a.test_mode, a.slide_crop, a.slide_stride, a.flip, a.max_views_per_call) == ("val", "whole", None, None, False, 16)
    assert (a.eval, a.out, a.format_only, a.imgfile_prefix, a.show_dir, a.opacity, a.palette) == (True, "", False, "", "", 0.5, "")
    assert a.val_split == "val" and T.get_args(CKPT + ["--eval", "--split", "test"]).val_split == "test"
    # the model and data flags are run_semseg's, with its defaults and derived values
    r = R.get_args([])
    for k in ("data_root", "vit", "embed_dim", "num_heads", "depth", "out_indices", "net_size", "drop", "num_classes", "decode_channels",
              "aux_channels", "pool_scales", "canvas", "crop_size", "ratio_range", "slice_max_evs", "samples_per_gpu", "workers_per_gpu"):
        assert getattr(a, k) == getattr(r, k), k
    s = T.get_args(CKPT + ["--out", "r.pkl", "--test_mode", "slide", "--slide_crop", "32", "32", "--slide_stride", "16", "24", "--flip"])
    assert (s.test_mode, s.slide_crop, s.slide_stride, s.flip, s.eval, s.out) == ("slide", [32, 32], [16, 24], True, False, "r.pkl")
    with pytest.raises(SystemExit):
        T.get_args(["--eval"])                                  # --checkpoint is required


def test_tool_refusals_by_name():
    from mem_amd import infer_semseg as T
    with pytest.raises(NotImplementedError, match="--flip is its flip half") as e:
        T.get_args(CKPT + ["--eval", "--aug-test"])
    assert "multi-scale" in str(e.value) and "misaligned with the label" in str(e.value) and "dsec.py:36-44" in str(e.value)
    for flags, needle in ((["--launcher", "pytorch"], "--launcher pytorch"), (["--distributed"], "--distributed"),
                          (["--world_size", "2"], "--world_size 2"), (["--gpus", "2"], "--gpus 2"),
                          (["--gpu-collect"], "--gpu_collect"), (["--cat_max_ratio", "0.75"], "--cat_max_ratio")):
        with pytest.raises(NotImplementedError, match=needle):
            T.get_args(CKPT + ["--eval"] + flags)
    for flags, needle in ((["--eval", "--test_mode", "slide"], "--slide_crop"),
                          (["--eval", "--test_mode", "slide", "--slide_crop", "32", "32"], "--slide_stride"),
                          (["--eval", "--slide_crop", "32", "32"], "--test_mode slide"),
                          ([], "nothing to do"), (["--eval", "--format-only", "--imgfile_prefix", "d"], "cannot both"),
                          (["--out", "r.json"], ".pkl"), (["--format-only"], "--imgfile_prefix"),
                          (["--show-dir", "d", "--opacity", "0"], "--opacity")):
        with pytest.raises(ValueError, match=needle):
            T.get_args(CKPT + flags)
    with pytest.raises(SystemExit):
        T.get_args(CKPT + ["--eval", "--test_mode", "tiles"])


def test_run_semseg_still_refuses_slide_and_aug_test():
    from mem_amd import run_semseg as R
    with pytest.raises(NotImplementedError, match="--test_mode slide"):
        R.get_args(["--test_mode", "slide"])
    with pytest.raises(NotImplementedError, match="--aug_test"):
        R.get_args(["--aug-test"])


class _Head:
    num_classes, align_corners = 5, False


class _Model:
    decode_head = _Head()


class _Pipe:
    def __init__(self, **kw):
        from mem_amd.seg_data import SegPipelineConfig
        self.cfg = SegPipelineConfig(**{**dict(canvas=(48, 64), img_scale=(48, 64), crop_size=(48, 64), net_size=(96, 128), y_limit=48), **kw})


def test_inferencer_views_and_refusals():
    from mem_amd.seg_infer import SegInferencer
    inf = SegInferencer(_Model(), _Pipe(), mode="slide", crop_size=(32, 32), stride=(16, 24), flip=True)
    assert inf.rects[:6] == GRID and inf.rects[6:] == [(y, x, 1) for y, x, _ in GRID]
    assert inf.records[:6] == GRID and inf.records[6:] == [(y, 64 - x - 32, 1) for y, x, _ in GRID]       # left = W - x1 - wc
    assert inf.describe() == {"test_mode": "slide", "windows": 6, "crop": [32, 32], "stride": [16, 24], "flip": True}
    whole = SegInferencer(_Model(), _Pipe())
    assert whole.rects == [(0, 0, 0)] and whole.window == (48, 64) and whole.evaluator.num_classes == 5
    with pytest.raises(ValueError, match="crop_size=.* and stride="):
        SegInferencer(_Model(), _Pipe(), mode="slide", crop_size=(32, 32))
    with pytest.raises(ValueError, match="crop_size=.* and stride="):
        SegInferencer(_Model(), _Pipe(), mode="slide", stride=(8, 8))
    with pytest.raises(NotImplementedError, match="larger than the canvas"):
        SegInferencer(_Model(), _Pipe(), mode="slide", crop_size=(49, 32), stride=(8, 8))
    with pytest.raises(NotImplementedError, match="differs from the canvas"):
        SegInferencer(_Model(), _Pipe(img_scale=(96, 128)))
    with pytest.raises(NotImplementedError, match="differs from the canvas"):
        SegInferencer(_Model(), _Pipe(crop_size=(32, 64)))
    with pytest.raises(NotImplementedError, match="align_corners=True"):
        SegInferencer(_Model(), _Pipe(), align_corners=True)
    with pytest.raises(NotImplementedError, match="at most 64"):
        SegInferencer(_Model(), _Pipe(), mode="slide", crop_size=(8, 8), stride=(8, 8), flip=True)         # 6 x 8 x 2 views
    with pytest.raises(ValueError, match="mode="):
        SegInferencer(_Model(), _Pipe(), mode="tiles")


# ---------------------------------------------------------------- palette and painter
def test_default_palette_is_deterministic_and_distinct():
    from mem_amd.seg_infer import default_palette
    p = default_palette(32)
    assert p.dtype == torch.uint8 and tuple(p.shape) == (32, 3) and torch.equal(p, default_palette(32))
    assert torch.equal(default_palette(11), p[:11])                              # a class keeps its colour
    assert len({tuple(c) for c in default_palette(64).tolist()}) == 64
    d = (p[:, None, :].int() - p[None, :, :].int()).abs().sum(-1)
    assert int((d + 1000 * torch.eye(32, dtype=torch.int32)).min()) >= 24            # no two of 32 classes look alike
    assert tuple(default_palette(0).shape) == (0, 3)


def test_paint_is_the_blend_truncated():
    from mem_amd.seg_infer import default_palette, paint
    g = torch.Generator().manual_seed(0)
    pred = torch.randint(0, 11, (2, 5, 7), generator=g, dtype=torch.uint8)
    image = torch.randint(0, 256, (2, 5, 7, 3), generator=g, dtype=torch.uint8)
    pal = default_palette(11)
    for opacity in (0.5, 0.3, 1.0):
        want = (image.numpy().astype(np.float64) * (1 - opacity) + pal.numpy()[pred.numpy()].astype(np.float64) * opacity).astype(np.uint8)
        got = paint(pred, image, pal, opacity)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 5, 7, 3) and np.array_equal(got.numpy(), want)
    assert torch.equal(paint(pred, image, pal, 1.0), pal[pred.long()])
    with pytest.raises(ValueError, match="no colour"):
        paint(pred, image, pal[:5], 0.5)
    with pytest.raises(ValueError, match=r"\[B, H, W, 3\]"):
        paint(pred, image.permute(0, 3, 1, 2), pal, 0.5)
    with pytest.raises(ValueError, match="opacity"):
        paint(pred, image, pal, 0.0)
