"""-m "not gpu": the host side of the segmentation loss (csrc/seg_plan.cpp, mem_amd/seg_loss.py).

Axis tables against torch's own CPU bilinear interpolation in float64 (interpolating the identity matrix reads off the
weights), the plan's tiles / footprints / LDS / workspace over a grid of shapes, the refusals of the struct entry points
without a device, the layout of memhip_seg_args_t / memhip_seg_plan_t against the header as the host compiler lays them out,
and SegEvaluator.compute() on a hand-written confusion matrix."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "memhip.h")
P = 0x1000          # a dummy, aligned, non-NULL address: nothing is dereferenced before a launch


# ---------------------------------------------------------------- axis tables
def _torch_weights(n_in, n_out, align):
    """[out, in] float64: row y holds the weights with which torch's bilinear resize reads the inputs for output y"""
    eye = torch.eye(n_in, dtype=torch.float64).reshape(1, n_in, n_in, 1)            # channel k = the k-th unit vector, along H
    out = F.interpolate(eye, size=(n_out, 1), mode="bilinear", align_corners=bool(align))
    return out[0, :, :, 0].t().numpy()


CASES = [(n_in, n_out, align) for n_in in range(1, 13) for n_out in range(n_in, 5 * n_in + 1) for align in (0, 1)]


def test_axis_tables_reproduce_torch_and_ranges_are_exact():
    from mem_amd import ops
    for n_in, n_out, align in CASES:
        i0, w1, lo, hi = ops.seg_axis_table(n_in, n_out, align)
        i1 = np.minimum(i0 + 1, n_in - 1)
        assert i0.min() >= 0 and i0.max() <= n_in - 1, (n_in, n_out, align)
        assert np.all(w1 >= 0) and np.all(w1 <= 1.0 + 1e-6), (n_in, n_out, align)
        # the weights: scatter (1 - w1) to i0 and w1 to i1, compare with torch's float64 rows
        mine = np.zeros((n_out, n_in))
        ys = np.arange(n_out)
        np.add.at(mine, (ys, i0), 1.0 - w1.astype(np.float64))
        np.add.at(mine, (ys, i1), w1.astype(np.float64))
        want = _torch_weights(n_in, n_out, align)
        assert np.abs(mine - want).max() <= 1e-6, (n_in, n_out, align, np.abs(mine - want).max())
        # the index: identical wherever w1 is not within 1e-6 of 0 or 1 (there a unit weight may sit on either neighbour)
        for y in ys:
            if 1e-6 < w1[y] < 1.0 - 1e-6:
                nz = np.nonzero(want[y] > 1e-9)[0]
                assert list(nz) == sorted({i0[y], i1[y]}), (n_in, n_out, align, y, nz, i0[y])
        # lo / hi: exactly the outputs that read input i through i0 or i1; contiguous, monotone
        for i in range(n_in):
            touching = np.nonzero((i0 == i) | (i1 == i))[0]
            assert len(touching) > 0, (n_in, n_out, align, i)
            assert (lo[i], hi[i]) == (touching[0], touching[-1]), (n_in, n_out, align, i)
            assert len(touching) == hi[i] - lo[i] + 1, (n_in, n_out, align, i, "not contiguous")
        assert np.all(np.diff(lo) >= 0) and np.all(np.diff(hi) >= 0) and np.all(np.diff(i0) >= 0), (n_in, n_out, align)
        assert lo[0] == 0 and hi[-1] == n_out - 1


def test_every_output_has_exactly_one_home():
    """home = the tile of i0: over the tiles of an axis the sets {y: first <= i0[y] <= last} partition the outputs, and each
    lies inside that tile's footprint lo[first] .. hi[last]"""
    from mem_amd import ops
    for n_in, n_out, align in CASES + [(17, 68, 0), (23, 57, 1), (110, 440, 0)]:
        i0, _, lo, hi = ops.seg_axis_table(n_in, n_out, align)
        homes = np.zeros(n_out, np.int64)
        for first in range(0, n_in, 8):
            last = min(first + 8, n_in) - 1
            mine = np.nonzero((i0 >= first) & (i0 <= last))[0]
            homes[mine] += 1
            assert len(mine) == 0 or (mine[0] >= lo[first] and mine[-1] <= hi[last])
        assert np.all(homes == 1), (n_in, n_out, align)


def test_axis_table_refusals():
    from mem_amd import _lib, ops
    for n_in, n_out, align, msg in ((0, 4, 0, "bad shape in=0 out=4"), (5, 4, 0, "bad shape in=5 out=4"), (2, 4, 2, "align_corners=2")):
        with pytest.raises(_lib.MemhipError, match=re.escape(msg)):
            ops.seg_axis_table(n_in, n_out, align)
    assert _lib.lib.memhip_seg_axis_table(2, 4, 0, None, None, None, None) == -1
    assert b"null pointer" in _lib.lib.memhip_last_error()


# ---------------------------------------------------------------- plan
SIDES = [(1, 1), (1, 4), (2, 2), (3, 7), (7, 9), (8, 32), (9, 36), (15, 16), (16, 64), (17, 68), (13, 29), (23, 23), (31, 97),
         (110, 440), (1, 4096)]
PLAN_SHAPES = [(B, Cc, h, w, H, W) for (B, Cc) in ((1, 2), (3, 11), (2, 19), (16, 32))
               for (h, H), (w, W) in itertools.product(SIDES, SIDES) if (h + w + Cc) % 3 != 1 or (h, w) in ((1, 1), (110, 110))]


def test_plan_tiles_footprints_lds_and_workspace():
    from mem_amd import ops
    assert len(PLAN_SHAPES) > 300
    for B, Cc, h, w, H, W in PLAN_SHAPES:
        for align in (0, 1):
            p = ops.seg_plan(B, Cc, h, w, H, W, align)
            # tiles cover h x w exactly once
            cover = np.zeros((h, w), np.int64)
            for ty in range(p.tiles_y):
                for tx in range(p.tiles_x):
                    cover[ty * p.tile_h:(ty + 1) * p.tile_h, tx * p.tile_w:(tx + 1) * p.tile_w] += 1
            assert np.all(cover == 1), (h, w)
            assert (p.tiles_y - 1) * p.tile_h < h and (p.tiles_x - 1) * p.tile_w < w, "an empty tile"
            assert p.grid == B * p.tiles_y * p.tiles_x and p.block == 256 and p.chunk == p.block
            # footprints: every output that reads a pixel of a tile is inside lo[first] .. hi[last], which the plan's maximum bounds
            for n_in, n_out, tile, max_f in ((h, H, p.tile_h, p.max_fh), (w, W, p.tile_w, p.max_fw)):
                i0, _, lo, hi = ops.seg_axis_table(n_in, n_out, align)
                i1 = np.minimum(i0 + 1, n_in - 1)
                widest = 0
                for first in range(0, n_in, tile):
                    last = min(first + tile, n_in) - 1
                    touching = np.nonzero(((i0 >= first) & (i0 <= last)) | ((i1 >= first) & (i1 <= last)))[0]
                    assert touching[0] >= lo[first] and touching[-1] <= hi[last]
                    # and what it reads lies in the tile plus one pixel around it
                    inside = np.arange(lo[first], hi[last] + 1)
                    assert i0[inside].min() >= first - 1 and i1[inside].max() <= last + 1
                    widest = max(widest, hi[last] - lo[first] + 1)
                assert max_f == widest, (n_in, n_out, align, max_f, widest)
            # LDS: the halo tile of logits, one chunk of q for every (padded) channel, the tables when they are staged
            cp = max(8, (Cc + 3) // 4 * 4)
            fixed = ((p.tile_h + 2) * (p.tile_w + 2) * (cp + 1) + cp * p.chunk) * 4
            tables = (p.max_fh + p.max_fw) * 8
            assert p.lds_bytes == fixed + (tables if p.tables_in_lds else 0)
            assert p.lds_bytes <= 64 * 1024
            assert p.tables_in_lds == int(fixed + tables <= 64 * 1024)
            assert fixed >= p.block * (8 + 3 * 4), "the workgroup's fold reuses the q chunk"
            # workspace: one slot per workgroup
            assert p.slot_bytes == 24 and p.ws_bytes >= p.grid * p.slot_bytes
            assert 1 <= p.conf_grid <= 2048 and p.conf_grid * p.conf_block >= min(B * H * W, 2048 * 256)
            assert p.conf_lds_bytes >= Cc * Cc * 4


# ---------------------------------------------------------------- refusals without a device
def _args(**kw):
    """a complete, acceptable struct on dummy addresses, with the given fields replaced"""
    from mem_amd import ops
    shape = dict(B=2, C_=11, h=9, w=17, H=36, W=68, ignore_index=255, align_corners=False, avg_non_ignore=False, loss_weight=1.0)
    fields = dict(logits=P, labels=P, dz=P, loss=P, stats=P, workspace=P, workspace_bytes=1 << 30, confusion=P,
                  y_i0=P, y_w1=P, y_lo=P, y_hi=P, x_i0=P, x_w1=P, x_lo=P, x_hi=P)
    for k, v in kw.items():
        (shape if k in shape else fields)[k] = v
    return ops.seg_args(**shape, **fields)


def _call(fn, a):
    from mem_amd import _lib
    rc = getattr(_lib.lib, fn)(None if a is None else C.byref(a), None)
    return rc, _lib.lib.memhip_last_error().decode()


def test_refusals_name_the_fault_and_the_query_agrees():
    from mem_amd import _lib, ops
    shape_cases = [(dict(C_=1), "seg: bad shape C=1 (2 <= C <= 32)"), (dict(C_=33), "seg: bad shape C=33 (2 <= C <= 32)"),
                   (dict(H=8), "seg: bad shape H=8 W=68 for logits of 9x17"), (dict(W=16), "seg: bad shape H=36 W=16 for logits of 9x17"),
                   (dict(B=0), "seg: bad shape B=0"), (dict(h=0), "seg: bad shape h=0 w=17"),
                   (dict(H=40000), "too many pixels"), (dict(ignore_index=256), "seg: ignore_index=256"),
                   (dict(align_corners=2), "seg: align_corners=2"), (dict(avg_non_ignore=3), "seg: avg_non_ignore=3")]
    for fn in ("memhip_seg_ce", "memhip_seg_confusion"):
        assert _call(fn, None) == (-1, "seg: null args")
        for kw, msg in shape_cases:
            rc, err = _call(fn, _args(**kw))
            assert rc == -1 and msg in err, (fn, kw, rc, err)
            plan = ops.SegPlan()
            rc_q = _lib.lib.memhip_seg_plan(C.byref(_args(**kw)), C.byref(plan))
            assert (rc_q, _lib.lib.memhip_last_error().decode()) == (rc, err)
        for field in ("logits", "labels"):
            rc, err = _call(fn, _args(**{field: None}))
            assert rc == -1 and "seg: null pointer (logits, labels)" in err, (fn, field, err)
        for field in ("y_i0", "y_w1", "y_lo", "y_hi", "x_i0", "x_w1", "x_lo", "x_hi"):
            rc, err = _call(fn, _args(**{field: None}))
            assert rc == -1 and "seg: null pointer (axis tables)" in err, (fn, field, err)
    for field in ("dz", "loss", "stats", "workspace"):
        rc, err = _call("memhip_seg_ce", _args(**{field: None}))
        assert rc == -1 and "seg_ce: null pointer" in err, (field, err)
    rc, err = _call("memhip_seg_ce", _args(workspace=P + 4))
    assert rc == -1 and "not 8-byte aligned" in err
    rc, err = _call("memhip_seg_ce", _args(loss_weight=float("inf")))
    assert rc == -1 and "loss_weight" in err
    rc, err = _call("memhip_seg_confusion", _args(confusion=None))
    assert rc == -1 and "seg_confusion: null pointer" in err
    # the workspace: too small is its own code, by the call and by a query that is given one
    need = ops.seg_plan(2, 11, 9, 17, 36, 68).ws_bytes
    assert need == 2 * 2 * 3 * 24
    rc, err = _call("memhip_seg_ce", _args(workspace_bytes=need - 1))
    assert rc == -2 and "workspace %d < %d" % (need - 1, need) in err
    assert _lib.lib.memhip_seg_plan(C.byref(_args(workspace_bytes=need - 1)), C.byref(ops.SegPlan())) == -2
    assert _lib.lib.memhip_seg_plan(C.byref(_args(workspace=None, workspace_bytes=0)), C.byref(ops.SegPlan())) == 0
    assert _lib.lib.memhip_seg_plan(C.byref(_args()), None) == -1
    # the query asks about a call it does not make: no pointer needed
    assert _lib.lib.memhip_seg_plan(C.byref(ops.seg_args(2, 11, 9, 17, 36, 68)), C.byref(ops.SegPlan())) == 0


def test_cpu_tensors_raise():
    from mem_amd import _lib
    from mem_amd.seg_loss import SegCrossEntropy, SegEvaluator
    z, lab = torch.zeros(1, 3, 2, 2), torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(_lib.MemhipError, match="no CPU fallback"):
        SegCrossEntropy()(z, lab)
    with pytest.raises(_lib.MemhipError, match="no CPU fallback"):
        SegEvaluator(3).update(z, lab)


# ---------------------------------------------------------------- struct layout
def _seg_structs():
    """{typedef name: [fields]} of the two tagged structs of the segmentation section"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for tag, body in re.findall(r"^struct\s+(memhip_seg_\w+)\s*\{(.*?)\n\};", src, flags=re.S | re.M):
        assert re.search(r"typedef\s+struct\s+%s\s+%s_t\s*;" % (tag, tag), src), tag
        fields = []
        for decl in body.split(";"):
            for piece in decl.split(","):
                piece = re.sub(r"\[[^\]]*\]", "", piece).strip()
                if piece:
                    fields.append(re.findall(r"\w+", piece)[-1])
        out[tag + "_t"] = fields
    return out


def test_seg_struct_layout_matches_header(tmp_path):
    from mem_amd import ops
    mirrors = {"memhip_seg_args_t": ops.SegArgs, "memhip_seg_plan_t": ops.SegPlan}
    structs = _seg_structs()
    assert set(structs) == set(mirrors)
    cc = next((c for c in (shutil.which("cc"), "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang") if c and os.path.exists(c)), None)
    if cc is None:
        pytest.skip("no host C compiler")
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "memhip.h"', "int main(void) {"]
    for name, fields in structs.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f in fields]
    lines += ["  return 0;", "}"]
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    open(src, "w").write("\n".join(lines) + "\n")
    r = subprocess.run([cc, "-I", os.path.dirname(HEADER), src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    printed = dict(re.findall(r"^(\S+) (\d+)$", subprocess.run([exe], capture_output=True, text=True, check=True).stdout, re.M))
    for name, fields in structs.items():
        cls = mirrors[name]
        assert [f[0] for f in cls._fields_] == fields, (name, "field names / order differ from the header")
        assert C.sizeof(cls) == int(printed[name]), (name, C.sizeof(cls), printed[name])
        for f in fields:
            assert getattr(cls, f).offset == int(printed[name + "." + f]), (name, f)


# ---------------------------------------------------------------- metrics
def test_evaluator_compute_on_a_hand_written_matrix_with_an_absent_class():
    from mem_amd.seg_loss import SegEvaluator, metrics_from_confusion
    # row = label, column = prediction.  Class 2 never occurs and is never predicted; class 3 never occurs but is predicted.
    m = torch.tensor([[6, 1, 0, 1],
                      [2, 8, 0, 0],
                      [0, 0, 0, 0],
                      [0, 0, 0, 0]], dtype=torch.int64)
    ev = SegEvaluator(4)
    ev.matrix = m.clone()
    r = ev.compute()
    assert r["aAcc"] == pytest.approx(14 / 18)
    iou = r["IoU"].numpy()
    assert iou[0] == pytest.approx(6 / (8 + 8 - 6)) and iou[1] == pytest.approx(8 / (10 + 9 - 8))
    assert np.isnan(iou[2]) and iou[3] == 0.0
    acc = r["Acc"].numpy()
    assert acc[0] == pytest.approx(6 / 8) and acc[1] == pytest.approx(8 / 10) and np.isnan(acc[2]) and np.isnan(acc[3])
    assert r["mIoU"] == pytest.approx((0.6 + 8 / 11 + 0.0) / 3)
    assert r["mAcc"] == pytest.approx((0.75 + 0.8) / 2)
    # merge adds, reset clears, the reduce hook is used on request
    other = SegEvaluator(4)
    other.matrix = m.clone()
    ev.merge(other)
    assert torch.equal(ev.matrix, 2 * m) and ev.compute()["mIoU"] == pytest.approx(r["mIoU"])
    calls = []
    ev.reduce = lambda mat: (calls.append(1), mat * 3)[1]
    assert ev.compute(reduce=True)["aAcc"] == pytest.approx(14 / 18) and calls == [1] and torch.equal(ev.matrix, 2 * m)
    ev.reset()
    assert int(ev.matrix.sum()) == 0
    assert metrics_from_confusion(m)["mAcc"] == pytest.approx(r["mAcc"])
