"""The DSEC segmentation data pipeline, batched on the GPU -- mirror of the two mmseg pipelines of
mem/semantic_segmentation/configs/_base_/datasets/dsec.py with the transforms of
mem/semantic_segmentation/backbone/EventDataset.py and the backbone's own ``resize_in`` (backbone/mem.py:294,420).

Split of work, as in ``mem_amd.augment``:
  * WORKERS, per sample, CPU only (``EventSegDataset``): load the ``.npy`` events and the ``.png`` label, p -> 2p - 1, the
    ``y < 440`` cut, ``SliceRandomMaxEvs(180000)`` on the kept rows (LoadNpy, EventDataset.py:737-746, in that order), and every
    random DRAW of the chain as one small record (``draw_seg_sample``).  Nothing is rasterized, resized or augmented there.
  * DEVICE, per batch (``SegBatchPipeline``): events -> ``memhip_rasterize`` (u8 counts that wrap at 256, as EventArrToImg's
    u8 ``np.add.at``) -> ``memhip_segdata_resize_hist`` (Resize + the histograms) -> ``memhip_segdata_norm`` (RemoveHotPixelsEvs,
    NormalizeEvs, ToUnit8Evs) -> in training ``memhip_rand_augment_u8`` twice, once per group of equal size
    (EventRandAugmentEvs) -> ``memhip_segdata_geom`` (RandomCrop, RandomFlip, Normalize(to_rgb), Pad, resize_in; for the label
    the nearest Resize, the same crop and flip, Pad 255).  Nothing synchronises with the host.

The draws equal the reference's in distribution, not in stream: there they come from ``np.random``, ``random`` and
``torch.randint`` of each DataLoader worker.  Here one ``numpy.random.Generator`` per sample makes all of them, in the order of
``DRAW_DTYPE``.  Not mirrored: ``cat_max_ratio < 1`` (class-balanced crops), multi-scale / flip test-time augmentation, an
antialiased ``resize_in`` (``antialias=True`` is refused: the tensor behaviour current when the reference was written is taken).
"""
import os

import numpy as np
import torch

from . import ops
from .augment import RANDAUG_DTYPE, randaug_record

# EventRandAugmentEvs(no_geometric_trafos=True): EventDataset.py:1426-1437, in the dict's order
SEG_RANDAUG_OPS = ["Identity", "Brightness", "Color", "Contrast", "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize"]

# One sample's draws, in the order they are made: the start of the event slice (SliceRandomMaxEvs; 0 when nothing is cut), the
# ratio of Resize, then per RandAugment op (index into SEG_RANDAUG_OPS, magnitude bin, sign), then RandomCrop's top and left and
# RandomFlip's decision.
DRAW_DTYPE = np.dtype([("start", "<i8"), ("ratio", "<f8"), ("ra", [("op", "<i4"), ("bin", "<i4"), ("sign", "<i4")], (2,)),
                       ("top", "<i4"), ("left", "<i4"), ("flip", "<i4")])


class SegPipelineConfig:
    """The values of dsec.py and of LoadNpy; sizes are (h, w)."""

    def __init__(self, canvas=(440, 640), img_scale=(440, 640), ratio_range=(1.0, 1.01), crop_size=(440, 640), net_size=(512, 512),
                 slice_max=180000, y_limit=440, num_stds=10.0, ra_num_ops=2, ra_magnitude=10, ra_bins=31, flip_ratio=0.5,
                 cat_max_ratio=1.0, seg_pad_val=255, antialias=False):
        if antialias:
            raise NotImplementedError("antialias=True: resize_in is F.interpolate's bilinear without antialias, as when the "
                                      "reference was written (torchvision >= 0.17 would antialias the 640 -> 512 downscale)")
        if cat_max_ratio < 1.0:
            raise NotImplementedError(f"cat_max_ratio={cat_max_ratio}: class-balanced crops are not mirrored (dsec.py sets 1.0)")
        if ra_num_ops != 2:
            raise NotImplementedError(f"ra_num_ops={ra_num_ops}: the draw record holds the reference's two ops")
        if seg_pad_val != 255:
            raise NotImplementedError(f"seg_pad_val={seg_pad_val}: the label kernel pads with 255, SegCrossEntropy's ignore_index")
        if not 1.0 <= ratio_range[0] <= ratio_range[1]:
            raise ValueError(f"ratio_range={ratio_range!r}: 1 <= min <= max (the resize of this pipeline never shrinks)")
        if not 0 <= ra_magnitude < ra_bins:
            raise ValueError(f"ra_magnitude={ra_magnitude}: 0 .. ra_bins - 1")
        self.canvas, self.img_scale, self.crop_size = tuple(canvas), tuple(img_scale), tuple(crop_size)
        self.net_size = tuple(net_size)
        self.ratio_range = (float(ratio_range[0]), float(ratio_range[1]))
        self.slice_max, self.y_limit, self.num_stds = int(slice_max), int(y_limit), float(num_stds)
        self.ra_num_ops, self.ra_magnitude, self.ra_bins = int(ra_num_ops), int(ra_magnitude), int(ra_bins)
        self.flip_ratio, self.cat_max_ratio, self.seg_pad_val = float(flip_ratio), float(cat_max_ratio), int(seg_pad_val)

    def dims_of(self, ratio):
        """mmseg's Resize.random_sample_ratio: (int(h * ratio), int(w * ratio)), both from the same ratio."""
        return int(self.img_scale[0] * ratio), int(self.img_scale[1] * ratio)

    def max_dims(self):
        return self.dims_of(self.ratio_range[1])


def _ra_magnitudes(num_bins):
    """EventDataset.py:1426-1437 as float64 arrays (torch.linspace in fp32 there; the record keeps fp32)."""
    import torch as t
    lin = t.linspace(0.0, 0.9, num_bins)
    return {"Identity": (None, False), "Brightness": (lin, True), "Color": (lin, True), "Contrast": (lin, True),
            "Sharpness": (lin, True), "Posterize": (8 - (t.arange(num_bins) / ((num_bins - 1) / 4)).round().int(), False),
            "Solarize": (t.linspace(255.0, 0.0, num_bins), False), "AutoContrast": (None, False), "Equalize": (None, False)}


def draw_seg_sample(cfg, n_events, rng, train):
    """Every random decision of one sample as a DRAW_DTYPE record, drawn from ``rng`` (a numpy Generator) in the record's
    order.  ``n_events``: the rows left after the y cut.  The test pipeline slices at random too (LoadNpy is in both), resizes
    with ratio 1, and neither augments, crops at an offset nor flips (MyMultiScaleFlipAug(flip=False) sets the decision)."""
    d = np.zeros((), dtype=DRAW_DTYPE)
    if n_events > cfg.slice_max:                                       # SliceRandomMaxEvs, EventDataset.py:622-626
        d["start"] = int(rng.integers(0, n_events - cfg.slice_max + 1))
    d["ratio"] = 1.0
    if not train:
        return d
    lo, hi = cfg.ratio_range
    d["ratio"] = rng.random() * (hi - lo) + lo                         # mmseg Resize.random_sample_ratio
    for k in range(cfg.ra_num_ops):                                    # EventRandAugmentEvs.forward, EventDataset.py:1477-1484
        d["ra"][k]["op"] = int(rng.integers(0, len(SEG_RANDAUG_OPS)))
        d["ra"][k]["bin"] = int(rng.integers(0, cfg.ra_magnitude + 1))
        d["ra"][k]["sign"] = int(rng.integers(0, 2))
    h, w = cfg.dims_of(float(d["ratio"]))
    d["top"] = int(rng.integers(0, max(h - cfg.crop_size[0], 0) + 1))  # mmseg RandomCrop.get_crop_bbox
    d["left"] = int(rng.integers(0, max(w - cfg.crop_size[1], 0) + 1))
    d["flip"] = int(rng.random() < cfg.flip_ratio)                     # mmseg RandomFlip
    return d


def randaug_of(cfg, ra):
    """One (op, bin, sign) of a draw -> (name, magnitude), EventDataset.py:1479-1492."""
    name = SEG_RANDAUG_OPS[int(ra["op"])]
    mags, signed = _ra_magnitudes(cfg.ra_bins)[name]
    m = float(mags[int(ra["bin"])].item()) if mags is not None else 0.0
    if signed and int(ra["sign"]):
        m *= -1.0
    return name, m


def pair_files(root, split):
    """[(events .npy, label .png)] of ``imgs/<split>`` and ``anns/<split>``, sorted by the event file's name as
    EventDataset.load_annotations does (EventDataset.py:195-206); the label is the same relative path with the other suffix."""
    img_dir, ann_dir = os.path.join(root, "imgs", split), os.path.join(root, "anns", split)
    if not os.path.isdir(img_dir):
        raise FileNotFoundError(f"{img_dir}: no such folder")
    names = []
    for base, _, files in os.walk(img_dir):
        names += [os.path.relpath(os.path.join(base, f), img_dir) for f in files if f.endswith(".npy")]
    names.sort()
    pairs = []
    for n in names:
        ann = os.path.join(ann_dir, n[:-len(".npy")] + ".png")
        if not os.path.isfile(ann):
            raise FileNotFoundError(f"{ann}: the label of {os.path.join(img_dir, n)} is missing")
        pairs.append((os.path.join(img_dir, n), ann))
    return pairs


DSEC_CLASSES = ("background", "building", "fence", "person", "pole", "road", "sidewalk", "vegetation", "car", "wall",
                "traffic sign")


class EventSegDataset(torch.utils.data.Dataset):
    """``root/imgs/<split>/*.npy`` (events [n, 4] = x, y, t, p with p in {0, 1}) with ``root/anns/<split>/*.png`` (u8 class
    maps) and the class names of ``root/labels.txt`` (one per line).  ``root="synthetic"``: ``n_synthetic`` procedural samples on
    ``cfg.canvas`` (rectangles of classes; the event rate of a pixel follows its class, rows beyond the y cut included), for
    tests and benchmarks.

    ``dataset[i]`` or ``dataset[(i, seed)]`` -> ``(events f64 [n, 4], label u8 [H, W], draw)``: CPU only, safe in DataLoader
    workers.  The draws of a sample come from ``numpy.random.default_rng([self.seed, seed, i])``, so a run is repeatable and a
    resumed run continues its sequence (``IterBatchSampler`` hands out the seeds)."""

    def __init__(self, root, split, cfg=None, train=None, seed=0, n_synthetic=32, synthetic_events=20000, num_classes=11):
        self.cfg = cfg if cfg is not None else SegPipelineConfig()
        self.root, self.split, self.seed = root, split, int(seed)
        self.train = (split == "train") if train is None else bool(train)
        self.synthetic = root == "synthetic"
        if self.synthetic:
            self.pairs = [None] * int(n_synthetic)
            self.synthetic_events = int(synthetic_events)
            self.CLASSES = tuple(DSEC_CLASSES[:num_classes]) if num_classes <= len(DSEC_CLASSES) else \
                tuple("class%d" % i for i in range(num_classes))
        else:
            self.pairs = pair_files(root, split)
            with open(os.path.join(root, "labels.txt")) as f:
                self.CLASSES = tuple(line.strip() for line in f if line.strip())

    def __len__(self):
        return len(self.pairs)

    def _synthetic(self, i):
        H, W = self.cfg.canvas
        K = len(self.CLASSES)
        rng = np.random.default_rng([1234 if self.train else 4321, i])
        label = np.full((H, W), int(rng.integers(0, K)), dtype=np.uint8)
        for _ in range(6):
            y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            y1, x1 = min(H, y0 + int(rng.integers(H // 8 + 1, H // 2 + 2))), min(W, x0 + int(rng.integers(W // 8 + 1, W // 2 + 2)))
            label[y0:y1, x0:x1] = int(rng.integers(0, K))
        label[:, : max(1, W // 40)] = 255                                  # an ignored band, as DSEC's labels have
        n = self.synthetic_events
        # rejection sampling on the class' rate: class k keeps a candidate event with probability (k + 1) / K
        x = rng.integers(0, W, 3 * n)
        y = rng.integers(0, H + H // 11 + 1, 3 * n)                        # the sensor is taller than the labelled canvas
        cls = np.where(y < H, label[np.minimum(y, H - 1), x], 0).astype(np.int64) % K
        keep = np.flatnonzero(rng.random(3 * n) * K < cls + 1)[:n]
        x, y, cls = x[keep], y[keep], cls[keep]
        t = np.sort(rng.integers(0, 50000, len(keep)))
        p = (rng.random(len(keep)) < 0.25 + 0.5 * (cls % 2)).astype(np.int64)     # the polarity mix follows the class too
        return np.stack([x, y, t, p], 1).astype(np.float32), label

    def load(self, i):
        """(raw events f32 [n, 4] with p in {0, 1}, label u8 [H, W])"""
        if self.synthetic:
            return self._synthetic(i)
        from PIL import Image
        ev_path, ann_path = self.pairs[i]
        ev = np.load(ev_path).astype(np.float32)                           # LoadNpy, EventDataset.py:737
        label = np.asarray(Image.open(ann_path))
        if label.ndim != 2 or label.dtype != np.uint8:
            raise ValueError(f"{ann_path}: a single-channel 8-bit class map is expected, got {label.shape} {label.dtype}")
        return ev, np.ascontiguousarray(label)

    def __getitem__(self, key):
        i, seed = key if isinstance(key, tuple) else (key, 0)
        cfg = self.cfg
        ev, label = self.load(int(i))
        ev[:, 3] = 2 * ev[:, 3] - 1                                        # :738
        ev = ev[ev[:, 1] < cfg.y_limit]                                    # :740-741
        draw = draw_seg_sample(cfg, len(ev), np.random.default_rng([self.seed, int(seed), int(i)]), self.train)
        if len(ev) > cfg.slice_max:                                        # :742 SliceRandomMaxEvs on the kept rows
            ev = ev[int(draw["start"]): int(draw["start"]) + cfg.slice_max]
        if tuple(label.shape) != cfg.canvas:
            raise ValueError(f"sample {i}: label {label.shape} is not the canvas {cfg.canvas}")
        return ev.astype(np.float64), label, draw

    @staticmethod
    def collate(batch):
        """-> (events f64 [N, 4], offsets i64 [B + 1], labels u8 [B, H, W], draws DRAW_DTYPE [B]) as CPU tensors / arrays"""
        evs, labels, draws = zip(*batch)
        offsets = np.concatenate([[0], np.cumsum([len(e) for e in evs])]).astype(np.int64)
        return (torch.from_numpy(np.concatenate(evs, 0)), torch.from_numpy(offsets), torch.from_numpy(np.stack(labels)),
                np.stack(draws))


class IterBatchSampler:
    """Batches of ``(index, seed)`` keys for iteration-based training: iteration ``it`` takes the next ``batch`` indices of
    an endless sequence of seeded permutations (shuffle=True, dsec.py:53) and gives its samples the draw seed ``it``; starting
    at ``start_iter`` continues the sequence where a run of that many iterations stopped."""

    def __init__(self, n, batch, seed, start_iter, max_iters, shuffle=True):
        self.n, self.batch, self.seed, self.start_iter, self.max_iters, self.shuffle = n, batch, seed, start_iter, max_iters, shuffle

    def __len__(self):
        return max(0, self.max_iters - self.start_iter)

    def _perm(self, epoch):
        return np.random.default_rng([self.seed, epoch]).permutation(self.n) if self.shuffle else np.arange(self.n)

    def __iter__(self):
        for it in range(self.start_iter, self.max_iters):
            pos = it * self.batch
            keys = []
            while len(keys) < self.batch:
                epoch, off = divmod(pos, self.n)
                take = self._perm(epoch)[off: off + self.batch - len(keys)]
                keys += [(int(i), it) for i in take]
                pos += len(take)
            yield keys


class SegBatchPipeline:
    """``(events, offsets, labels, draws, train)`` -> ``(img f32 [B, 3, S_h, S_w], label u8 [B, crop_h, crop_w])`` on the device.

    events f64 [N, 4] and offsets i64 [B + 1] (CSR), labels u8 [B, H, W] or None, draws DRAW_DTYPE [B]; tensors on the CPU are
    uploaded.  A batch is ordered by drawn size inside the working buffer, so every group of equal size is one dense
    ``[n_g, 3, h, w]`` tensor for ``memhip_rand_augment_u8``; the outputs keep the batch's order.  Every buffer, the outputs
    included, is allocated once per shape and reused by the next call.  ``stages`` (``return_stages=True``) holds views of the
    intermediate buffers."""

    def __init__(self, cfg=None, device="cuda"):
        self.cfg = cfg if cfg is not None else SegPipelineConfig()
        self.device = torch.device(device)
        self._bufs = {}

    def _buf(self, name, shape, dtype):
        key = (name, tuple(shape), dtype)
        t = self._bufs.get(key)
        if t is None:
            t = self._bufs[key] = torch.empty(shape, dtype=dtype, device=self.device)
        return t

    def pack(self, draws, train):
        """Host: the draws -> (dims i32 [B, 2], offs i64 [B], crop i32 [B, 3], groups [(first element, (h, w), [samples])],
        RandAugment records [ops, B] in the buffer's order or None)."""
        cfg = self.cfg
        B = len(draws)
        dims = np.array([cfg.dims_of(float(d["ratio"])) for d in draws], dtype=np.int32).reshape(B, 2)
        order = sorted(range(B), key=lambda b: (int(dims[b, 0]), int(dims[b, 1]), b))
        offs = np.zeros(B, dtype=np.int64)
        groups, pos = [], 0
        for b in order:
            hw = (int(dims[b, 0]), int(dims[b, 1]))
            if not groups or groups[-1][1] != hw:
                groups.append((pos, hw, []))
            groups[-1][2].append(b)
            offs[b] = pos
            pos += 3 * hw[0] * hw[1]
        crop = np.array([(int(d["top"]), int(d["left"]), int(d["flip"])) for d in draws], dtype=np.int32).reshape(B, 3)
        ra = None
        if train:
            ra = np.zeros((cfg.ra_num_ops, B), dtype=RANDAUG_DTYPE)
            for slot, b in enumerate(order):
                for k in range(cfg.ra_num_ops):
                    ra[k, slot] = randaug_record(*randaug_of(cfg, draws[b]["ra"][k]))
        return dims, offs, crop, groups, ra, pos

    def __call__(self, events, offsets, labels, draws, train, return_stages=False):
        from ._lib import C, check, lib, ptr, stream_ptr
        from .datasets import raster_args, raster_run
        cfg, dev = self.cfg, self.device
        B = len(draws)
        H, W = cfg.canvas
        mh, mw = cfg.max_dims()
        dims_h, offs_h, crop_h, groups, ra_h, used = self.pack(draws, train)
        # one upload for the small records: offs | dims | crop | RandAugment records, each part 8-byte aligned
        parts = [offs_h.view(np.uint8).reshape(-1), dims_h.view(np.uint8).reshape(-1), crop_h.view(np.uint8).reshape(-1)]
        if ra_h is not None:
            parts.append(ra_h.view(np.uint8).reshape(-1))
        starts, blob = [], bytearray()
        for p in parts:
            blob += b"\0" * (-len(blob) % 8)
            starts.append(len(blob))
            blob += p.tobytes()
        rec = torch.frombuffer(blob, dtype=torch.uint8).to(dev, non_blocking=True)
        offs = rec[starts[0]: starts[0] + 8 * B].view(torch.int64)
        dims = rec[starts[1]: starts[1] + 8 * B].view(torch.int32).view(B, 2)
        crop = rec[starts[2]: starts[2] + 12 * B].view(torch.int32).view(B, 3)
        events = events.to(dev, non_blocking=True)
        offsets = offsets.to(dev, non_blocking=True)
        if labels is not None:
            labels = labels.to(dev, non_blocking=True).contiguous()
        # EventArrToImg(440, 640): [pos, 0, neg] u8 planes, counts mod 256
        planes = self._buf("planes", (B, 3, H, W), torch.uint8)
        status = self._buf("status", (B,), torch.int32)
        raster_run(raster_args(B, H, W, False, n_events=int(events.shape[0]), ev=ptr(events), offsets=ptr(offsets), out=ptr(planes),
                               status=ptr(status)), dev)
        cap = B * 3 * mh * mw
        img = self._buf("img", (cap,), torch.uint8)
        hist = self._buf("hist", (B, 2, 256), torch.int32)
        ops.segdata_resize_hist(planes, offs, dims, (mh, mw), img, hist)
        stages = {"planes": planes, "status": status, "dims": dims, "offs": offs, "hist": hist}
        if train:
            ops.segdata_norm(offs, dims, (mh, mw), img, hist, cfg.num_stds)
            other = self._buf("img2", (cap,), torch.uint8)
            ra = rec[starts[3]:].view(cfg.ra_num_ops, B * RANDAUG_DTYPE.itemsize)
            st = stream_ptr()
            for k in range(cfg.ra_num_ops):                                  # img -> other -> img
                slot = 0
                for first, (h, w), members in groups:
                    n = len(members)
                    check(lib.memhip_rand_augment_u8(C.c_void_p(img.data_ptr() + first), C.c_void_p(other.data_ptr() + first),
                                                     C.c_void_p(ra[k].data_ptr() + slot * RANDAUG_DTYPE.itemsize), n, h, w, st),
                          "rand_augment")
                    slot += n
                img, other = other, img
            assert cfg.ra_num_ops % 2 == 0                                   # the result is back in the "img" buffer
            src = img
        else:
            src = self._buf("imgf", (cap,), torch.float32)
            ops.segdata_norm(offs, dims, (mh, mw), img, hist, cfg.num_stds, img_f32=src)
        out = self._buf("out", (B, 3) + cfg.net_size, torch.float32)
        label_out = self._buf("label", (B,) + cfg.crop_size, torch.uint8) if labels is not None else None
        ops.segdata_geom(offs, dims, (mh, mw), src, crop, cfg.crop_size, cfg.net_size, out=out, labels=labels, label_out=label_out)
        self.last_status = status
        if return_stages:
            stages.update(img=src, groups=groups, used=used)
            return out, label_out, stages
        return out, label_out
