"""-m "not gpu": the host side of the segmentation data chain (mem_amd/seg_data.py, memhip_segdata_args_t): the layout of the
args struct against its ctypes mirror, the entries' argument checks in front of any launch, draw ranges and draw order, file
pairing, the batch's packing by size, the synthetic source and the refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "memhip.h")


# ---------------------------------------------------------------------------------------------- ABI
def _header_fields():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"struct\s+memhip_segdata_args\s*\{(.*?)\}\s*;", src, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        for piece in decl.split(","):
            piece = piece.strip()
            if piece:
                fields.append(re.findall(r"\w+", piece)[-1])
    return fields


def test_args_struct_layout_matches_the_ctypes_mirror(tmp_path):
    from mem_amd import ops
    from test_abi_layout_cpu import _host_cc
    cc = _host_cc()
    assert cc is not None, "no host C compiler"
    fields = _header_fields()
    assert fields == [f[0] for f in ops.SegDataArgs._fields_], "field names / order differ from the header"
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "memhip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(memhip_segdata_args_t));']
    lines += ['  printf("%s %%zu\\n", offsetof(memhip_segdata_args_t, %s));' % (f, f) for f in fields]
    lines += ["  return 0;", "}"]
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    open(src, "w").write("\n".join(lines) + "\n")
    r = subprocess.run([cc, "-I", os.path.dirname(HEADER), src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    printed = dict(re.findall(r"^(\w+) (\d+)$", subprocess.run([exe], capture_output=True, text=True, check=True).stdout, re.M))
    assert C.sizeof(ops.SegDataArgs) == int(printed.pop("size"))
    for f in fields:
        assert getattr(ops.SegDataArgs, f).offset == int(printed[f]), f


def test_entries_resolve_and_the_abi_number_stays():
    """the three entries are additive (no existing signature changed), so the number stays, as for every addition since 10"""
    from mem_amd import _lib
    assert _lib.ABI_VERSION == _lib.lib.memhip_abi_version() == 10
    header = open(HEADER).read()
    for name in ("memhip_segdata_resize_hist", "memhip_segdata_norm", "memhip_segdata_geom"):
        assert getattr(_lib.lib, name) and f"int {name}(const memhip_segdata_args_t* args, memhip_stream_t stream);" in header


P = 0x1000


def _args(**kw):
    from mem_amd import ops
    base = dict(B=2, H=12, W=20, max_h=13, max_w=22, crop_h=12, crop_w=20, net_h=16, net_w=16, num_stds=10.0, planes=P, offs=P,
                dims=P, img_u8=P, img_f32=P, img_elems=4096, hist=P, crop=P, out=P, labels=P, label_out=P)
    base.update(kw)
    return ops.SegDataArgs(**base)


def _rejected(fn, a, text):
    from mem_amd import _lib
    rc = getattr(_lib.lib, fn)(None if a is None else C.byref(a), None)
    msg = _lib.lib.memhip_last_error().decode()
    assert rc == -1 and text in msg, (fn, rc, msg)


def test_entries_check_their_arguments_before_any_launch():
    """Dummy addresses: every case is rejected by the host checks, nothing is dereferenced or launched."""
    for fn in ("memhip_segdata_resize_hist", "memhip_segdata_norm", "memhip_segdata_geom"):
        _rejected(fn, None, "null args")
        _rejected(fn, _args(B=-1), "B=-1")
        _rejected(fn, _args(max_h=0), "max_h=0")
        _rejected(fn, _args(max_w=5000), "max_w=5000")
        _rejected(fn, _args(img_elems=-1), "img_elems")
        _rejected(fn, _args(offs=None), "offs and dims")
        _rejected(fn, _args(dims=None), "offs and dims")
    _rejected("memhip_segdata_resize_hist", _args(H=0), "H=0")
    _rejected("memhip_segdata_resize_hist", _args(planes=None), "planes, img_u8 and hist")
    _rejected("memhip_segdata_resize_hist", _args(hist=None), "planes, img_u8 and hist")
    _rejected("memhip_segdata_norm", _args(out_f32=2), "out_f32=2")
    _rejected("memhip_segdata_norm", _args(num_stds=-1.0), "num_stds")
    _rejected("memhip_segdata_norm", _args(out_f32=1, img_f32=None), "out_f32 needs img_f32")
    _rejected("memhip_segdata_norm", _args(img_u8=None), "img_u8 and hist")
    _rejected("memhip_segdata_geom", _args(crop_h=0), "crop_h=0")
    _rejected("memhip_segdata_geom", _args(net_w=0), "net_w=0")
    _rejected("memhip_segdata_geom", _args(in_f32=3), "in_f32=3")
    _rejected("memhip_segdata_geom", _args(in_f32=1, img_f32=None), "in_f32 selects")
    _rejected("memhip_segdata_geom", _args(img_u8=None), "in_f32 selects")
    _rejected("memhip_segdata_geom", _args(labels=None), "label_out needs labels")
    _rejected("memhip_segdata_geom", _args(out=None, label_out=None), "neither out nor label_out")


def test_empty_batch_is_ok_and_reads_nothing():
    from mem_amd import _lib
    for fn in ("memhip_segdata_resize_hist", "memhip_segdata_norm", "memhip_segdata_geom"):
        a = _args(B=0, planes=None, offs=None, dims=None, img_u8=None, img_f32=None, hist=None, crop=None, labels=None)
        assert getattr(_lib.lib, fn)(C.byref(a), None) == 0, fn


# ---------------------------------------------------------------------------------------------- draws
def test_config_defaults_are_the_reference_values():
    from mem_amd.seg_data import SegPipelineConfig
    c = SegPipelineConfig()
    assert (c.canvas, c.img_scale, c.crop_size, c.net_size) == ((440, 640), (440, 640), (440, 640), (512, 512))
    assert c.ratio_range == (1.0, 1.01) and c.slice_max == 180000 and c.y_limit == 440 and c.num_stds == 10.0
    assert (c.ra_num_ops, c.ra_magnitude, c.ra_bins, c.flip_ratio, c.cat_max_ratio, c.seg_pad_val) == (2, 10, 31, 0.5, 1.0, 255)
    assert c.dims_of(1.0) == (440, 640) and c.max_dims() == (444, 646) and c.dims_of(1.005) == (442, 643)


def test_draw_ranges():
    from mem_amd.seg_data import DRAW_DTYPE, SEG_RANDAUG_OPS, SegPipelineConfig, draw_seg_sample
    cfg = SegPipelineConfig()
    rng = np.random.default_rng(7)
    n = 200000
    ds = np.stack([draw_seg_sample(cfg, n, rng, True) for _ in range(4000)])
    assert ds.dtype == DRAW_DTYPE
    assert ds["start"].min() >= 0 and ds["start"].max() <= n - 180000 and ds["start"].max() > 15000
    assert ds["ratio"].min() >= 1.0 and ds["ratio"].max() < 1.01
    dims = np.array([cfg.dims_of(r) for r in ds["ratio"]])
    assert set(dims[:, 0]) == set(range(440, 445)) and set(dims[:, 1]) == set(range(640, 647))
    assert set(ds["ra"]["op"].ravel()) == set(range(len(SEG_RANDAUG_OPS))) and len(SEG_RANDAUG_OPS) == 9
    assert set(ds["ra"]["bin"].ravel()) == set(range(11)) and set(ds["ra"]["sign"].ravel()) == {0, 1}
    assert (ds["top"] >= 0).all() and (ds["top"] <= dims[:, 0] - 440).all() and ds["top"].max() == 4
    assert (ds["left"] >= 0).all() and (ds["left"] <= dims[:, 1] - 640).all() and ds["left"].max() == 6
    assert set(ds["flip"]) == {0, 1} and 0.45 < ds["flip"].mean() < 0.55
    # nothing to slice: start stays 0
    assert int(draw_seg_sample(cfg, 180000, rng, True)["start"]) == 0
    # the test pipeline: a random slice, and nothing else
    t = np.stack([draw_seg_sample(cfg, n, rng, False) for _ in range(50)])
    assert t["start"].max() > 0 and (t["ratio"] == 1.0).all() and not t["ra"]["op"].any() and not t["top"].any() \
        and not t["left"].any() and not t["flip"].any()


class _Recorder:
    """stands in for a numpy Generator: records the order of the calls"""

    def __init__(self):
        self.calls = []

    def integers(self, lo, hi):
        self.calls.append(("integers", lo, hi))
        return lo

    def random(self):
        self.calls.append(("random",))
        return 0.5


def test_draw_order():
    """start, ratio, 2 x (op, magnitude bin, sign), top, left, flip -- the order of the record's fields"""
    from mem_amd.seg_data import DRAW_DTYPE, SegPipelineConfig, draw_seg_sample
    assert DRAW_DTYPE.names == ("start", "ratio", "ra", "top", "left", "flip")
    assert DRAW_DTYPE["ra"].base.names == ("op", "bin", "sign") and DRAW_DTYPE["ra"].shape == (2,)
    cfg = SegPipelineConfig()
    r = _Recorder()
    d = draw_seg_sample(cfg, 180010, r, True)
    ratio = 0.5 * (1.01 - 1.0) + 1.0
    h, w = cfg.dims_of(ratio)
    assert r.calls == [("integers", 0, 11), ("random",), ("integers", 0, 9), ("integers", 0, 11), ("integers", 0, 2),
                       ("integers", 0, 9), ("integers", 0, 11), ("integers", 0, 2), ("integers", 0, h - 440 + 1),
                       ("integers", 0, w - 640 + 1), ("random",)]
    assert float(d["ratio"]) == ratio and int(d["flip"]) == 0            # 0.5 < 0.5 is False
    r = _Recorder()
    draw_seg_sample(cfg, 1000, r, False)
    assert r.calls == []


def test_randaug_magnitudes_follow_the_reference_table():
    from mem_amd.augment import OPS
    from mem_amd.seg_data import SEG_RANDAUG_OPS, SegPipelineConfig, randaug_of
    cfg = SegPipelineConfig()
    assert set(SEG_RANDAUG_OPS) <= set(OPS) and not set(SEG_RANDAUG_OPS) & {"ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"}
    rec = np.zeros((), dtype=[("op", "<i4"), ("bin", "<i4"), ("sign", "<i4")])
    rec["op"], rec["bin"], rec["sign"] = SEG_RANDAUG_OPS.index("Brightness"), 10, 1
    name, m = randaug_of(cfg, rec)
    assert name == "Brightness" and abs(m + 0.3) < 1e-6                   # linspace(0, 0.9, 31)[10], signed
    rec["op"], rec["sign"] = SEG_RANDAUG_OPS.index("Posterize"), 1
    assert randaug_of(cfg, rec) == ("Posterize", 7.0)                     # 8 - round(10 / 7.5); unsigned
    rec["op"], rec["bin"] = SEG_RANDAUG_OPS.index("Solarize"), 0
    assert randaug_of(cfg, rec) == ("Solarize", 255.0)
    rec["op"] = SEG_RANDAUG_OPS.index("Equalize")
    assert randaug_of(cfg, rec) == ("Equalize", 0.0)


# ---------------------------------------------------------------------------------------------- files
def _write_sample(root, split, stem, n=50, H=12, W=20, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "imgs", split, os.path.dirname(stem)), exist_ok=True)
    os.makedirs(os.path.join(root, "anns", split, os.path.dirname(stem)), exist_ok=True)
    ev = np.stack([rng.integers(0, W, n), rng.integers(0, H + 4, n), np.sort(rng.integers(0, 1000, n)), rng.integers(0, 2, n)], 1)
    np.save(os.path.join(root, "imgs", split, stem + ".npy"), ev.astype(np.int64))
    lab = rng.integers(0, 3, (H, W)).astype(np.uint8)
    Image.fromarray(lab).save(os.path.join(root, "anns", split, stem + ".png"))
    return ev, lab


def test_file_pairing_and_the_worker_side(tmp_path):
    from mem_amd.seg_data import EventSegDataset, SegPipelineConfig, pair_files
    root = str(tmp_path)
    written = {s: _write_sample(root, "train", s, seed=i) for i, s in enumerate(["b_000002", "a_000010", "a_000001", "sub/c_000000"])}
    open(os.path.join(root, "imgs", "train", "notes.txt"), "w").write("not a sample")
    open(os.path.join(root, "labels.txt"), "w").write("road\ncar\n\nperson\n")
    pairs = pair_files(root, "train")
    stems = [os.path.relpath(p[0], os.path.join(root, "imgs", "train"))[:-4] for p in pairs]
    assert stems == ["a_000001", "a_000010", "b_000002", "sub/c_000000"]       # sorted by file name, sub-folders included
    assert all(a.endswith(s + ".png") and os.path.join("anns", "train") in a for (_, a), s in zip(pairs, stems))
    cfg = SegPipelineConfig(canvas=(12, 20), img_scale=(12, 20), crop_size=(12, 20), net_size=(16, 16), slice_max=30, y_limit=12)
    ds = EventSegDataset(root, "train", cfg, seed=3)
    assert len(ds) == 4 and ds.CLASSES == ("road", "car", "person") and ds.train
    ev, lab, draw = ds[(1, 5)]
    raw, want_lab = written["a_000010"]
    assert np.array_equal(lab, want_lab) and ev.dtype == np.float64
    kept = raw[raw[:, 1] < 12].astype(np.float64)
    kept[:, 3] = 2 * kept[:, 3] - 1
    assert len(kept) > 30                                                       # the slice acts, on the KEPT rows
    s = int(draw["start"])
    assert 0 <= s <= len(kept) - 30 and np.array_equal(ev, kept[s:s + 30])
    assert set(np.unique(ev[:, 3])) <= {-1.0, 1.0} and ev[:, 1].max() < 12
    # the same key gives the same draws, another seed other ones
    again = ds[(1, 5)][2]
    assert again.tobytes() == draw.tobytes()
    assert any(ds[(1, k)][2].tobytes() != draw.tobytes() for k in range(6, 10))
    batch = ds.collate([ds[(0, 0)], ds[(3, 0)]])
    assert batch[1].tolist() == [0, 30, 60] and tuple(batch[0].shape) == (60, 4) and tuple(batch[2].shape) == (2, 12, 20)
    assert batch[3].shape == (2,)
    # a label without its events is fine; events without their label are not
    os.remove(os.path.join(root, "anns", "train", "b_000002.png"))
    with pytest.raises(FileNotFoundError, match="b_000002"):
        pair_files(root, "train")
    with pytest.raises(FileNotFoundError):
        pair_files(root, "val")


def test_synthetic_source():
    from mem_amd.seg_data import EventSegDataset, SegPipelineConfig
    cfg = SegPipelineConfig(canvas=(48, 64), img_scale=(48, 64), crop_size=(48, 64), net_size=(64, 96), slice_max=5000, y_limit=48)
    ds = EventSegDataset("synthetic", "train", cfg, n_synthetic=5, synthetic_events=8000, num_classes=11)
    assert len(ds) == 5 and len(ds.CLASSES) == 11
    raw, _ = ds.load(2)
    assert raw[:, 1].max() >= 48 and set(np.unique(raw[:, 3])) == {0.0, 1.0}      # rows beyond the cut exist, p in {0, 1}
    ev, lab, draw = ds[(2, 1)]
    assert lab.shape == (48, 64) and lab.dtype == np.uint8 and (lab[:, 0] == 255).all()
    assert set(np.unique(lab)) - {255} <= set(range(11)) and len(np.unique(lab)) > 2
    assert len(ev) == 5000 and ev[:, 1].max() < 48 and ev[:, 0].max() < 64 and (np.diff(ev[:, 2]) >= 0).all()
    assert np.array_equal(ds[(2, 1)][0], ev)
    val = EventSegDataset("synthetic", "val", cfg, n_synthetic=5, synthetic_events=8000)
    assert not val.train and not np.array_equal(val.load(2)[1], ds.load(2)[1])


def test_iter_batch_sampler_resumes_its_sequence():
    from mem_amd.seg_data import IterBatchSampler
    full = list(IterBatchSampler(5, 2, seed=1, start_iter=0, max_iters=9))
    assert len(full) == 9 and all(len(b) == 2 for b in full)
    assert [k[1] for b in full for k in b] == [i // 2 for i in range(18)]        # the draw seed is the iteration
    idx = [k[0] for b in full for k in b]
    assert sorted(idx[:5]) == sorted(idx[5:10]) == list(range(5)) and idx[:5] != idx[5:10]
    assert list(IterBatchSampler(5, 2, seed=1, start_iter=4, max_iters=9)) == full[4:]
    assert len(IterBatchSampler(5, 2, 1, 9, 9)) == 0


def test_pack_orders_the_buffer_by_size():
    from mem_amd.augment import RANDAUG_DTYPE
    from mem_amd.seg_data import DRAW_DTYPE, SEG_RANDAUG_OPS, SegBatchPipeline, SegPipelineConfig
    cfg = SegPipelineConfig(canvas=(100, 200), img_scale=(100, 200), crop_size=(100, 200), net_size=(64, 64), ratio_range=(1.0, 1.02))
    draws = np.zeros(4, dtype=DRAW_DTYPE)
    draws["ratio"] = [1.01, 1.0, 1.01, 1.0]
    draws["ra"]["op"][:, 0] = [SEG_RANDAUG_OPS.index(n) for n in ("Solarize", "Identity", "Equalize", "Posterize")]
    draws["top"], draws["left"], draws["flip"] = [1, 0, 0, 0], [2, 0, 1, 0], [1, 0, 0, 1]
    pipe = SegBatchPipeline(cfg, device="cpu")
    dims, offs, crop, groups, ra, used = pipe.pack(draws, True)
    assert dims.tolist() == [[101, 202], [100, 200], [101, 202], [100, 200]]
    a, b = 3 * 100 * 200, 3 * 101 * 202
    assert offs.tolist() == [2 * a, 0, 2 * a + b, a] and used == 2 * a + 2 * b
    assert groups == [(0, (100, 200), [1, 3]), (2 * a, (101, 202), [0, 2])]
    assert crop.tolist() == [[1, 2, 1], [0, 0, 0], [0, 1, 0], [0, 0, 1]]
    assert ra.dtype == RANDAUG_DTYPE and ra.shape == (2, 4)
    from mem_amd.augment import OPS
    assert [OPS[i] for i in ra[0]["op"]] == ["Identity", "Posterize", "Solarize", "Equalize"]      # the buffer's order
    assert pipe.pack(draws, False)[4] is None


def test_refusals():
    from mem_amd.seg_data import SegPipelineConfig
    with pytest.raises(NotImplementedError, match="antialias"):
        SegPipelineConfig(antialias=True)
    with pytest.raises(NotImplementedError, match="cat_max_ratio"):
        SegPipelineConfig(cat_max_ratio=0.75)
    with pytest.raises(NotImplementedError, match="ra_num_ops"):
        SegPipelineConfig(ra_num_ops=3)
    with pytest.raises(NotImplementedError, match="seg_pad_val"):
        SegPipelineConfig(seg_pad_val=0)
    with pytest.raises(ValueError, match="ratio_range"):
        SegPipelineConfig(ratio_range=(0.5, 1.0))
