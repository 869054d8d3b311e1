"""-m gpu: the kernels of csrc/seg_data.hip and mem_amd.seg_data.SegBatchPipeline against numpy / torch CPU restatements.

resize_hist and the labels are integer arithmetic and are compared bit for bit; norm is one correctly rounded fp32 division and
one multiply and is compared bit for bit with torch's CPU fp32; the final bilinear gather is compared with a float64 evaluation
within 2e-4 absolute (values <= 255, about ten fp32 roundings of weights and products: 255 * 10 * 2^-24 = 1.5e-4)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GEOM_TOL = 2e-4


# ---------------------------------------------------------------------------------------------- restatements
def ref_taps(n_in, n_out):
    i = np.arange(n_out, dtype=np.int64)
    num = np.clip((2 * i + 1) * n_in - n_out, 0, (n_in - 1) * 2 * n_out)      # source position * 2 n_out, edges clamped
    i0 = num // (2 * n_out)
    return i0, np.minimum(i0 + 1, n_in - 1), num - i0 * 2 * n_out


def ref_resize(src, h, w):
    """src u8 [3, H, W] -> u8 [3, h, w]: bilinear, half-pixel centres, exact rational weights, round half up; integers only"""
    H, W = src.shape[1:]
    y0, y1, fy = ref_taps(H, h)
    x0, x1, fx = ref_taps(W, w)
    s = src.astype(np.int64)
    gy, gx = (2 * h - fy)[None, :, None], (2 * w - fx)[None, None, :]
    fy, fx = fy[None, :, None], fx[None, None, :]
    a, b = s[:, y0][:, :, x0], s[:, y0][:, :, x1]
    c, d = s[:, y1][:, :, x0], s[:, y1][:, :, x1]
    v = (gy * (gx * a + fx * b) + fy * (gx * c + fx * d) + 2 * w * h) // (4 * w * h)
    assert v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)


def ref_hists(img):
    """img u8 [3, h, w] -> (H_val, H_pmax)"""
    return (np.bincount(img[[0, 2]].ravel(), minlength=256), np.bincount(np.maximum(img[0], img[2]).ravel(), minlength=256))


def ref_threshold(img, num_stds):
    v = img[[0, 2]].astype(np.int64).ravel()
    n, s1, s2 = int(v.size), int(v.sum()), int((v * v).sum())
    mean = np.float64(s1) / np.float64(n)
    var = np.float64(n * s2 - s1 * s1) / (np.float64(n) * np.float64(n - 1))      # unbiased
    return float(mean + np.float64(num_stds) * np.sqrt(var))


def ref_norm(img, num_stds, f32):
    """RemoveHotPixelsEvs + NormalizeEvs (+ ToUnit8Evs): torch CPU fp32 ``x / m * 255.``"""
    thr = ref_threshold(img, num_stds)
    pmax = np.maximum(img[0], img[2])
    hot = pmax > thr
    x = img.copy()
    x[0][hot] = 0
    x[2][hot] = 0
    surv = pmax[~hot]
    m = int(surv.max()) if surv.size and surv.max() > 0 else 1
    t = torch.from_numpy(x).to(torch.float32) / float(m) * 255.
    return (t if f32 else t.to(torch.uint8)), hot, m


def ref_geom_image(img, top, left, flip, crop, net):
    """img [3, h, w] (u8 or f32) -> float64 [3, net_h, net_w]: crop, flip, channel swap, zero pad, F.interpolate in float64"""
    x = torch.as_tensor(np.asarray(img)).double()
    x = x[:, top:top + crop[0], left:left + crop[1]]
    if flip:
        x = x.flip(2)
    x = x[[2, 1, 0]]
    x = F.pad(x, (0, crop[1] - x.shape[2], 0, crop[0] - x.shape[1]), value=0.0)
    return F.interpolate(x[None], size=net, mode="bilinear", align_corners=False)[0]


def ref_geom_label(lab, h, w, top, left, flip, crop):
    """lab u8 [H, W] -> u8 [crop_h, crop_w]: nearest resize to (h, w), crop, flip, pad 255"""
    H, W = lab.shape
    sy = np.minimum(np.arange(h) * H // h, H - 1)
    sx = np.minimum(np.arange(w) * W // w, W - 1)
    x = lab[sy][:, sx][top:top + crop[0], left:left + crop[1]]
    if flip:
        x = x[:, ::-1]
    out = np.full(crop, 255, dtype=np.uint8)
    out[:x.shape[0], :x.shape[1]] = x
    return out


# ---------------------------------------------------------------------------------------------- helpers
def _layout(dims):
    """consecutive dense [3, h, w] images: (offs, total)"""
    offs, pos = [], 0
    for h, w in dims:
        offs.append(pos)
        pos += 3 * h * w
    return offs, pos


def _dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype).cuda()


def _resize_hist(planes, dims, max_hw):
    from mem_amd import ops
    offs, total = _layout(dims)
    img = torch.full((total + 64,), 0xAB, dtype=torch.uint8, device="cuda")          # 64 guard bytes behind the last image
    hist = torch.full((len(dims), 2, 256), -1, dtype=torch.int32, device="cuda")      # the call clears it
    o, d = _dev(offs, torch.int64), _dev(dims, torch.int32).view(-1, 2)
    ops.segdata_resize_hist(torch.as_tensor(planes).cuda(), o, d, max_hw, img[:total], hist)
    torch.cuda.synchronize()
    assert bool((img[total:] == 0xAB).all()), "wrote behind the buffer"
    return img[:total], hist, o, d, offs


def _images(buf, dims, offs):
    b = buf.cpu().numpy()
    return [b[o:o + 3 * h * w].reshape(3, h, w) for (h, w), o in zip(dims, offs)]


# ---------------------------------------------------------------------------------------------- resize_hist
def test_resize_hist_is_the_exact_integer_resize():
    rng = np.random.default_rng(0)
    planes = rng.integers(0, 256, (3, 3, 12, 20), dtype=np.uint8)
    dims = [(12, 20), (13, 21), (12, 22)]
    img, hist, _, _, offs = _resize_hist(planes, dims, (13, 22))
    got = _images(img, dims, offs)
    hist = hist.cpu().numpy()
    for b, (h, w) in enumerate(dims):
        want = ref_resize(planes[b], h, w)
        assert np.array_equal(got[b], want), (b, int((got[b] != want).sum()))
        hv, hp = ref_hists(got[b])                                                # of the kernel's own output
        assert np.array_equal(hist[b, 0], hv) and np.array_equal(hist[b, 1], hp), b
        assert hist[b, 0].sum() == 2 * h * w and hist[b, 1].sum() == h * w
    assert np.array_equal(got[0], planes[0])                                      # equal sizes: an exact copy
    assert not np.array_equal(ref_resize(planes[1], 13, 21)[:, :12, :20], planes[1])


def test_resize_hist_skips_a_sample_whose_dims_or_offset_break_the_bounds():
    from mem_amd import ops
    rng = np.random.default_rng(1)
    planes = torch.from_numpy(rng.integers(0, 256, (3, 3, 12, 20), dtype=np.uint8)).cuda()
    total = 3 * 3 * 13 * 22
    img = torch.full((total,), 0xCD, dtype=torch.uint8, device="cuda")
    hist = torch.zeros((3, 2, 256), dtype=torch.int32, device="cuda")
    dims = _dev([(14, 20), (12, 20), (12, 20)], torch.int32)                      # sample 0: h beyond max_h
    offs = _dev([0, 720, total - 100], torch.int64)                               # sample 2: would end behind the buffer
    ops.segdata_resize_hist(planes, offs, dims, (13, 22), img, hist)
    torch.cuda.synchronize()
    b = img.cpu().numpy()
    assert np.array_equal(b[720:1440].reshape(3, 12, 20), planes[1].cpu().numpy())
    assert (b[:720] == 0xCD).all() and (b[1440:] == 0xCD).all()
    assert int(hist[0].sum()) == 0 and int(hist[2].sum()) == 0 and int(hist[1, 1].sum()) == 240


def test_resize_hist_behind_the_rasterizer_with_a_count_that_wraps():
    """300 events on one pixel: EventArrToImg's u8 np.add.at leaves 300 - 256 = 44, and so does memhip_rasterize"""
    from mem_amd import datasets as D
    rng = np.random.default_rng(2)
    n = 400
    ev = np.stack([rng.integers(0, 20, n), rng.integers(0, 12, n), np.sort(rng.integers(0, 1000, n)), rng.integers(0, 2, n) * 2 - 1],
                  1).astype(np.float64)
    hot = np.tile(np.array([[5.0, 3.0, 500.0, 1.0]]), (300, 1))
    ev = np.concatenate([ev, hot])
    want = np.zeros((3, 12 * 20), dtype=np.uint8)
    x, y, p = ev[:, 0].astype(np.int64), ev[:, 1].astype(np.int64), ev[:, 3]
    np.add.at(want[0], x[p == 1] + 20 * y[p == 1], 1)
    np.add.at(want[2], x[p == -1] + 20 * y[p == -1], 1)
    want = want.reshape(3, 12, 20)
    assert int(((x == 5) & (y == 3) & (p == 1)).sum()) >= 300 and want[0, 3, 5] == (int(((x == 5) & (y == 3) & (p == 1)).sum()) - 256)
    planes = D.rasterize(torch.from_numpy(ev).cuda(), torch.tensor([0, len(ev)], dtype=torch.int64, device="cuda"), 12, 20, False)
    assert np.array_equal(planes[0].cpu().numpy(), want)
    dims = [(13, 21)]
    img, hist, _, _, offs = _resize_hist(planes, dims, (13, 22))
    got = _images(img, dims, offs)[0]
    assert np.array_equal(got, ref_resize(want, 13, 21))
    assert np.array_equal(hist[0, 0].cpu().numpy(), ref_hists(got)[0])


# ---------------------------------------------------------------------------------------------- norm
def _norm(planes, num_stds, f32):
    """resize_hist at equal sizes (a copy + the histograms), then norm"""
    from mem_amd import ops
    B, _, h, w = planes.shape
    dims = [(h, w)] * B
    img, hist, o, d, offs = _resize_hist(planes, dims, (h, w))
    imgf = torch.full((img.numel(),), float("nan"), device="cuda") if f32 else None
    before = img.clone()
    ops.segdata_norm(o, d, (h, w), img, hist, num_stds, img_f32=imgf)
    torch.cuda.synchronize()
    if f32:
        assert torch.equal(img, before)                                           # the u8 image is left alone
        b = imgf.cpu().numpy()
        return [b[k:k + 3 * h * w].reshape(3, h, w) for k in offs]
    return _images(img, dims, offs)


def test_norm_is_exhaustive_over_value_and_maximum():
    """for each m in 1 .. 255 an image holding 0 .. m: (v / m * 255).to(uint8) of torch's CPU fp32, bit for bit.  The values
    are near uniform on 0 .. m, so thr = mean + 10 std is about 3.4 m: no pixel is hot (asserted on the input)."""
    h = w = 16
    p = np.arange(h * w)
    planes = np.zeros((255, 3, h, w), dtype=np.uint8)
    for m in range(1, 256):
        planes[m - 1, 0] = (p % (m + 1)).reshape(h, w)
        planes[m - 1, 1] = ((p * 7) % (m + 1)).reshape(h, w)                      # scaled like the others
        planes[m - 1, 2] = ((m - p) % (m + 1)).reshape(h, w)
        assert ref_threshold(planes[m - 1], 10.0) > m and planes[m - 1, [0, 2]].max() == m
        assert set(range(m + 1)) <= set(planes[m - 1, 0].ravel()) | set(planes[m - 1, 2].ravel())
    got = _norm(planes, 10.0, False)
    gotf = _norm(planes, 10.0, True)
    for m in range(1, 256):
        x = torch.from_numpy(planes[m - 1]).to(torch.float32)
        want = x / float(m) * 255.
        assert np.array_equal(gotf[m - 1].view(np.int32), want.numpy().view(np.int32)), m
        assert np.array_equal(got[m - 1], want.to(torch.uint8).numpy()), m


def test_norm_removes_hot_pixels_in_both_polarities():
    rng = np.random.default_rng(3)
    planes = rng.integers(0, 4, (2, 3, 12, 20), dtype=np.uint8)
    planes[:, 1] = 0
    planes[0, 0, 2, 3], planes[0, 2, 2, 3] = 255, 2                               # hot in one polarity: both are zeroed
    planes[0, 0, 7, 7] = planes[0, 2, 7, 8] = 3
    planes[1] = 0                                                                 # an all-zero image stays zero (m = 1)
    thr = ref_threshold(planes[0], 10.0)
    assert 3 < thr < 255
    for f32 in (False, True):
        got = _norm(planes, 10.0, f32)
        want, hot, m = ref_norm(planes[0], 10.0, f32)
        assert hot.sum() == 1 and hot[2, 3] and m == 3                            # the maximum is taken from the survivors
        assert np.array_equal(got[0], want.numpy())
        assert got[0][0, 2, 3] == 0 and got[0][2, 2, 3] == 0 and got[0][0, 7, 7] == 255 and got[0][2, 7, 8] == 255
        assert not got[1].any()


def test_norm_keeps_a_value_exactly_at_the_threshold():
    """num_stds = 0: thr = mean = 2 exactly.  max(ch0, ch2) == 2 is kept (strict comparison), 4 is removed."""
    planes = np.zeros((1, 3, 12, 20), dtype=np.uint8)
    planes[0, 0] = 4
    planes[0, 0, 5, 5] = 2                                                        # pixel A: max 2 == thr, kept
    planes[0, 2, 6, 6] = 2                                                        # pixel B: ch0 = 4 > thr, both removed
    assert ref_threshold(planes[0], 0.0) == 2.0
    for f32 in (False, True):
        got = _norm(planes, 0.0, f32)[0]
        want, hot, m = ref_norm(planes[0], 0.0, f32)
        assert m == 2 and hot.sum() == 239 and not hot[5, 5] and hot[6, 6]
        assert np.array_equal(got, want.numpy())
        assert got[0, 5, 5] == 255 and got.sum() == 255


# ---------------------------------------------------------------------------------------------- geom
GEOM_DIMS = [(12, 20), (12, 20), (13, 22), (13, 22), (10, 18)]
GEOM_CROP = [(0, 0, 0), (0, 0, 1), (0, 0, 0), (1, 2, 1), (0, 0, 1)]              # top, left, flip; (1, 2) = the full margin


@pytest.mark.parametrize("net", [(16, 16), (8, 24)])
@pytest.mark.parametrize("f32", [False, True])
def test_geom_image_and_label(net, f32):
    from mem_amd import ops
    rng = np.random.default_rng(4)
    crop_size = (12, 20)
    offs, total = _layout(GEOM_DIMS)
    if f32:
        buf = (rng.random(total) * 255).astype(np.float32)
    else:
        buf = rng.integers(0, 256, total, dtype=np.uint8)
    imgs = [buf[o:o + 3 * h * w].reshape(3, h, w) for (h, w), o in zip(GEOM_DIMS, offs)]
    labels = rng.integers(0, 11, (5, 12, 20), dtype=np.uint8)
    out = torch.full((5, 3) + net, float("nan"), device="cuda")
    lab_out = torch.full((5,) + crop_size, 77, dtype=torch.uint8, device="cuda")
    ops.segdata_geom(_dev(offs, torch.int64), _dev(GEOM_DIMS, torch.int32), (13, 22), torch.from_numpy(buf).cuda(),
                     _dev(GEOM_CROP, torch.int32), crop_size, net, out=out, labels=torch.from_numpy(labels).cuda(), label_out=lab_out)
    torch.cuda.synchronize()
    worst = 0.0
    for b, ((h, w), (top, left, flip)) in enumerate(zip(GEOM_DIMS, GEOM_CROP)):
        want = ref_geom_image(imgs[b], top, left, flip, crop_size, net)
        err = float((out[b].cpu().double() - want).abs().max())
        worst = max(worst, err)
        assert err <= GEOM_TOL, (b, err)
        assert np.array_equal(lab_out[b].cpu().numpy(), ref_geom_label(labels[b], h, w, top, left, flip, crop_size)), b
    print("geom net %s f32 %s: largest image error %.3e (bound %.1e)" % (net, f32, worst, GEOM_TOL))
    # the padded sample: its label carries 255 outside 10 x 18, its image zeros at the far corner
    assert bool((lab_out[4, 10:] == 255).all()) and bool((lab_out[4, :, 18:] == 255).all())
    assert float(out[4, :, -1, -1].abs().max()) == 0.0
    # the channel swap shows: output channel 0 of the plain sample is input channel 2
    assert float((out[0, 0].cpu().double() - ref_geom_image(imgs[0], 0, 0, 0, crop_size, net)[0]).abs().max()) <= GEOM_TOL
    assert float((out[0, 0].cpu().double() - ref_geom_image(imgs[0][[2, 1, 0]], 0, 0, 0, crop_size, net)[0]).abs().max()) > 1.0


def test_geom_halves_can_be_off():
    from mem_amd import ops
    rng = np.random.default_rng(5)
    dims, crop = [(12, 20)], [(0, 0, 1)]
    buf = torch.from_numpy(rng.integers(0, 256, 720, dtype=np.uint8)).cuda()
    labels = torch.from_numpy(rng.integers(0, 11, (1, 12, 20), dtype=np.uint8)).cuda()
    o, d, c = _dev([0], torch.int64), _dev(dims, torch.int32), _dev(crop, torch.int32)
    out = torch.zeros((1, 3, 16, 16), device="cuda")
    ops.segdata_geom(o, d, (12, 20), buf, c, (12, 20), (16, 16), out=out)
    lab = torch.zeros((1, 12, 20), dtype=torch.uint8, device="cuda")
    ops.segdata_geom(o, d, (12, 20), None, c, (12, 20), labels=labels, label_out=lab)
    assert torch.equal(lab[0], labels[0].flip(1)) and float(out.abs().max()) > 0


# ---------------------------------------------------------------------------------------------- the whole pipeline
def _cpu_chain(cfg, ev, label, draw, train):
    """one sample through the reference's chain on the CPU: EventArrToImg, Resize (the integer form), RemoveHotPixelsEvs,
    NormalizeEvs, (ToUnit8Evs, RandAugment through the library's oracle-tested kernel), crop / flip / swap / pad, resize_in"""
    from mem_amd._lib import C, check, lib, stream_ptr
    from mem_amd.augment import randaug_record
    from mem_amd.seg_data import randaug_of
    H, W = cfg.canvas
    planes = np.zeros((3, H * W), dtype=np.uint8)
    x, y, p = ev[:, 0].astype(np.int64), ev[:, 1].astype(np.int64), ev[:, 3]
    np.add.at(planes[0], x[p == 1] + W * y[p == 1], 1)
    np.add.at(planes[2], x[p == -1] + W * y[p == -1], 1)
    h, w = cfg.dims_of(float(draw["ratio"]))
    img = ref_resize(planes.reshape(3, H, W), h, w)
    img = ref_norm(img, cfg.num_stds, not train)[0]
    if train:
        a = img.cuda().contiguous()[None]
        for k in range(2):
            rec = torch.from_numpy(np.frombuffer(randaug_record(*randaug_of(cfg, draw["ra"][k])).tobytes(), dtype=np.uint8).copy()).cuda()
            b = torch.empty_like(a)
            check(lib.memhip_rand_augment_u8(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(rec.data_ptr()), 1, h, w,
                                             stream_ptr()), "rand_augment")
            a = b
        img = a[0].cpu()
    top, left, flip = int(draw["top"]), int(draw["left"]), int(draw["flip"])
    return (ref_geom_image(img.numpy(), top, left, flip, cfg.crop_size, cfg.net_size),
            ref_geom_label(label, h, w, top, left, flip, cfg.crop_size))


@pytest.mark.parametrize("train", [True, False])
def test_pipeline_against_the_per_sample_chain(train):
    from mem_amd.seg_data import SEG_RANDAUG_OPS, EventSegDataset, SegBatchPipeline, SegPipelineConfig
    cfg = SegPipelineConfig(canvas=(48, 64), img_scale=(48, 64), crop_size=(48, 64), net_size=(64, 96), ratio_range=(1.0, 1.05),
                            slice_max=6000, y_limit=48)
    ds = EventSegDataset("synthetic", "train", cfg, train=train, n_synthetic=3, synthetic_events=9000)
    samples = [list(ds[(i, 0)]) for i in range(3)]
    if train:                                                                       # forced draws: two sizes, every branch
        forced = [dict(ratio=1.045, ops=("Contrast", "Equalize"), top=2, left=1, flip=1),
                  dict(ratio=1.0, ops=("Sharpness", "Solarize"), top=0, left=0, flip=0),
                  dict(ratio=1.045, ops=("Posterize", "AutoContrast"), top=0, left=2, flip=0)]
        for s, f in zip(samples, forced):
            d = s[2]
            d["ratio"], d["top"], d["left"], d["flip"] = f["ratio"], f["top"], f["left"], f["flip"]
            for k in range(2):
                d["ra"][k]["op"], d["ra"][k]["bin"], d["ra"][k]["sign"] = SEG_RANDAUG_OPS.index(f["ops"][k]), 7 + k, k
        assert cfg.dims_of(1.045) == (50, 66)
    # a hot pixel in sample 1: 150 events more on one pixel
    samples[1][0] = np.concatenate([samples[1][0], np.tile(np.array([[9.0, 7.0, 60000.0, 1.0]]), (150, 1))])
    events, offsets, labels, draws = ds.collate([tuple(s) for s in samples])
    pipe = SegBatchPipeline(cfg)
    img, lab, stages = pipe(events, offsets, labels, draws, train, return_stages=True)
    torch.cuda.synchronize()
    assert tuple(img.shape) == (3, 3, 64, 96) and img.dtype == torch.float32 and tuple(lab.shape) == (3, 48, 64)
    assert int(stages["status"].abs().sum()) == 0
    worst = 0.0
    for b, (ev, label, draw) in enumerate(samples):
        want_img, want_lab = _cpu_chain(cfg, ev, label, draw, train)
        assert np.array_equal(lab[b].cpu().numpy(), want_lab), b
        err = float((img[b].cpu().double() - want_img).abs().max())
        worst = max(worst, err)
        assert err <= GEOM_TOL, (b, err)
        assert float(img[b].abs().max()) > 0
    print("pipeline train=%s: largest image error %.3e (bound %.1e)" % (train, worst, GEOM_TOL))
    # a second call reuses every buffer and gives the same bits
    first = img.clone()
    img2, lab2 = pipe(events, offsets, labels, draws, train)
    assert img2.data_ptr() == img.data_ptr() and torch.equal(img2, first) and torch.equal(lab2, lab)
