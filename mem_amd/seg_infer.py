"""Segmentation inference: label maps from a trained ``SegModel``, whole-image or sliding-window, with flip averaging.

Mirror of mmseg 0.30 ``EncoderDecoder.slide_inference / whole_inference / inference / aug_test`` (reached from
configs/_base_/models/upernet_beit.py:53 and tools/test.py:94-99).  The chain is: the test data chain up to the normalised
image -> ``ops.segdata_geom`` cuts every view (a window of one flip state) and resizes it to the net size -> ``encode_decode``
over the stacked views -> ``ops.seg_predict`` gathers the label map.  No upsampled ``[B, C, H, W]`` tensor is written; torch
ops would write one per window and per flip.

Not carried, refused by name: multi-scale ratios, vertical flips, a canvas that differs from the label size, more than 64 views
per call, multi-GPU collection."""
import colorsys
import math

import numpy as np
import torch

from . import ops

MAX_VIEWS = 64                      # == the limit of memhip_seg_predict


def _axis_starts(size, crop, stride):
    grids = max(size - crop + stride - 1, 0) // stride + 1
    out = []
    for i in range(grids):
        y1 = i * stride
        y2 = min(y1 + crop, size)
        out.append(max(y2 - crop, 0))
    return out


def slide_windows(canvas, crop, stride):
    """mmseg's ``slide_inference`` grid: ``[(y1, x1)]`` of the windows of ``crop`` = (hc, wc) on ``canvas`` = (H, W) at
    ``stride`` = (sy, sx), row by row; the last row and the last column are pulled back inside the canvas."""
    (H, W), (hc, wc), (sy, sx) = canvas, crop, stride
    if hc < 1 or wc < 1 or sy < 1 or sx < 1:
        raise ValueError(f"slide_windows: crop {crop!r} and stride {stride!r} must be positive")
    return [(y1, x1) for y1 in _axis_starts(H, hc, sy) for x1 in _axis_starts(W, wc, sx)]


def default_palette(n):
    """A deterministic palette of ``n`` colours, u8 ``[n, 3]`` (r, g, b): class i takes the hue ``i`` golden-ratio steps round
    the colour wheel, with saturation and value cycling through three levels each, so neighbouring classes differ strongly
    and no two of the first 64 coincide."""
    out = []
    for i in range(int(n)):
        hue = (i * 0.6180339887498949) % 1.0
        sat = (0.85, 0.6, 1.0)[i % 3]
        val = (1.0, 0.8, 0.6)[(i // 3) % 3]
        out.append([int(c * 255.0 + 0.5) for c in colorsys.hsv_to_rgb(hue, sat, val)])
    return torch.tensor(out, dtype=torch.uint8).reshape(int(n), 3)


def paint(pred, image, palette, opacity=0.5):
    """mmseg's ``show_result``: u8 ``[B, H, W, 3]`` = ``image * (1 - opacity) + palette[pred] * opacity`` in float64, truncated.
    pred u8 / integer ``[B, H, W]``, image u8 ``[B, H, W, 3]``, palette u8 ``[n, 3]`` in the image's channel order; torch ops on
    the tensors' device (not a hot path)."""
    if not 0.0 < opacity <= 1.0:
        raise ValueError(f"paint: opacity={opacity} must be in (0, 1]")
    if image.dim() != 4 or image.shape[-1] != 3 or tuple(image.shape[:3]) != tuple(pred.shape):
        raise ValueError(f"paint: image {tuple(image.shape)} must be [B, H, W, 3] for pred {tuple(pred.shape)}")
    palette = torch.as_tensor(palette).to(pred.device)
    if int(pred.max()) >= palette.shape[0]:
        raise ValueError(f"paint: label {int(pred.max())} has no colour in a palette of {palette.shape[0]}")
    colour = palette[pred.long()].to(torch.float64)
    return (image.to(torch.float64) * (1.0 - opacity) + colour * opacity).to(torch.uint8)


class SegInferencer:
    """``predict(events, offsets, draws)`` -> label maps u8 ``[B, H, W]`` on the device.

    ``mode="whole"``: one view, the canvas.  ``mode="slide"``: the windows of ``slide_windows(canvas, crop_size, stride)``.
    ``flip=True`` adds the same views of the horizontally flipped canvas and averages the two passes' probabilities.  The
    ``V x B`` inputs run through ``model.encode_decode`` in chunks of at most ``max_views_per_call`` samples.  Buffers are per
    shape and reused: a returned tensor is valid until the next call with that batch size.  ``labels`` adds the batch to
    ``self.evaluator``'s confusion matrix (a ``SegEvaluator``: ``metrics_from_confusion`` and ``all_reduce_sum`` apply)."""

    def __init__(self, model, pipeline, mode="whole", crop_size=None, stride=None, flip=False, max_views_per_call=16,
                 align_corners=None, ignore_index=255):
        from .seg_loss import SegEvaluator
        cfg = pipeline.cfg
        head_ac = bool(getattr(model.decode_head, "align_corners", False))
        if align_corners is not None and bool(align_corners) != head_ac:
            raise NotImplementedError(f"align_corners={bool(align_corners)}: the decode head was built with align_corners={head_ac}; "
                                      "the tables give the last resize only, the head's own resizes would not follow")
        if mode not in ("whole", "slide"):
            raise ValueError(f"mode={mode!r}: 'whole' or 'slide'")
        if tuple(cfg.img_scale) != tuple(cfg.canvas):
            raise NotImplementedError(f"img_scale={cfg.img_scale} differs from the canvas {cfg.canvas}, the labels' size: the second "
                                      "resize to ori_shape is then not the identity and is not mirrored")
        H, W = cfg.canvas
        if mode == "slide":
            if crop_size is None or stride is None:
                raise ValueError("mode='slide' needs crop_size=(hc, wc) and stride=(sy, sx)")
            crop_size, stride = (int(crop_size[0]), int(crop_size[1])), (int(stride[0]), int(stride[1]))
            if crop_size[0] > H or crop_size[1] > W:
                raise NotImplementedError(f"crop_size={crop_size} is larger than the canvas {(H, W)}: mmseg pads the canvas "
                                          "and counts the padding, which is not mirrored")
            self.windows = slide_windows((H, W), crop_size, stride)
            self.window = crop_size
        else:
            if crop_size is not None or stride is not None:
                raise ValueError("mode='whole' takes no crop_size / stride")
            if tuple(cfg.crop_size) != (H, W):
                raise NotImplementedError(f"crop_size={cfg.crop_size} of the test chain differs from the canvas {(H, W)}, the "
                                          "labels' size: whole-image logits would not align with the label")
            self.windows = [(0, 0)]
            self.window = (H, W)
        if max_views_per_call < 1:
            raise ValueError(f"max_views_per_call={max_views_per_call}: at least 1")
        self.model, self.pipeline, self.mode, self.stride, self.flip = model, pipeline, mode, stride, bool(flip)
        self.canvas = (H, W)
        self.max_views_per_call = int(max_views_per_call)
        self.align_corners, self.ignore_index = head_ac, ignore_index
        hc, wc = self.window
        # (y1, x1, flip) for seg_predict; {top, left, flip} on the unflipped image for segdata_geom
        self.rects = [(y1, x1, 0) for y1, x1 in self.windows]
        self.records = [(y1, x1, 0) for y1, x1 in self.windows]
        if self.flip:
            self.rects += [(y1, x1, 1) for y1, x1 in self.windows]
            self.records += [(y1, W - x1 - wc, 1) for y1, x1 in self.windows]
        if len(self.rects) > MAX_VIEWS:
            raise NotImplementedError(f"{len(self.rects)} views (windows x flips): memhip_seg_predict takes at most {MAX_VIEWS}")
        self.num_classes = int(model.decode_head.num_classes)
        self.evaluator = SegEvaluator(self.num_classes, ignore_index, head_ac)
        self._bufs = {}
        self.last_image = None

    def _buf(self, name, shape, dtype, device):
        key = (name, tuple(shape), dtype)
        t = self._bufs.get(key)
        if t is None:
            t = self._bufs[key] = torch.empty(shape, dtype=dtype, device=device)
        return t

    def _records(self, B, device):
        key = ("records", B)
        t = self._bufs.get(key)
        if t is None:
            host = np.repeat(np.asarray(self.records, dtype=np.int32)[:, None, :], B, axis=1)
            t = self._bufs[key] = torch.from_numpy(np.ascontiguousarray(host)).to(device)
        return t

    @torch.no_grad()
    def view_logits(self, events, offsets, draws):
        """Steps 1 to 4: the logits of every view, ``[V B, C, h, w]`` (a view of the head's buffer when one model call took
        them all, else the stacked buffer), and the stages of the data chain."""
        cfg = self.pipeline.cfg
        B = len(draws)
        H, W = self.canvas
        if any(float(d["ratio"]) != 1.0 or int(d["flip"]) != 0 for d in draws):
            raise NotImplementedError("a draw with ratio != 1 or a flip: the test chain resizes with ratio 1 and does not flip "
                                      "(multi-scale ratios are not mirrored)")
        _, _, st = self.pipeline(events, offsets, None, draws, train=False, return_stages=True)
        dev = st["img"].device
        V = len(self.records)
        records = self._records(B, dev)
        inp = self._buf("inp", (V * B, 3) + tuple(cfg.net_size), torch.float32, dev)
        for v in range(V):
            ops.segdata_geom(st["offs"], st["dims"], cfg.max_dims(), st["img"], records[v], self.window, cfg.net_size,
                             out=inp[v * B: (v + 1) * B])
        n = V * B
        step = self.max_views_per_call
        if n <= step:
            return self.model.encode_decode(inp), st
        stacked = None
        for s in range(0, n, step):
            part = self.model.encode_decode(inp[s: s + step])
            if stacked is None:
                stacked = self._buf("logits", (n,) + tuple(part.shape[1:]), torch.float32, dev)
            stacked[s: s + part.shape[0]].copy_(part)
        return stacked, st

    @torch.no_grad()
    def predict(self, events, offsets, draws, labels=None, return_prob=False):
        """-> pred u8 ``[B, H, W]``, or ``(pred, prob f32 [B, C, H, W])``.  labels u8 ``[B, H, W]`` (the canvas' size): the batch
        is added to the confusion matrix in the same launch."""
        B = len(draws)
        H, W = self.canvas
        logits, st = self.view_logits(events, offsets, draws)
        dev = logits.device
        kw = {}
        if labels is not None:
            if tuple(labels.shape) != (B, H, W):
                raise NotImplementedError(f"labels {tuple(labels.shape)} differ from the canvas {(B, H, W)}: the second resize to "
                                          "ori_shape is then not the identity and is not mirrored")
            kw = dict(labels=labels.to(dev, non_blocking=True).contiguous(), confusion=self.evaluator._matrix(dev))
        pred = self._buf("pred", (B, H, W), torch.uint8, dev)
        prob = self._buf("prob", (B, self.num_classes, H, W), torch.float32, dev) if return_prob else None
        ops.seg_predict(logits, self.rects, self.window, (H, W), pred=pred, prob=prob, align_corners=self.align_corners,
                        ignore_index=self.ignore_index, **kw)
        self.last_image = st["img"][: B * 3 * H * W].view(B, 3, H, W)
        return (pred, prob) if return_prob else pred

    def image_u8(self):
        """The normalised event image of the last batch as u8 ``[B, H, W, 3]`` (channels as the data chain holds them: positive
        events, zero, negative events), for ``paint``."""
        return self.last_image.clamp(0.0, 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    def describe(self):
        return {"test_mode": self.mode, "windows": len(self.windows), "crop": list(self.window),
                "stride": list(self.stride) if self.stride else None, "flip": self.flip}

    @torch.no_grad()
    def evaluate(self, dataset, samples_per_gpu, workers, on_batch=None):
        """The dictionary ``run_semseg.evaluate`` returns, from this inferencer's label maps.  ``on_batch(indices, pred)`` sees
        every batch's label maps (valid during the call) in dataset order."""
        from .run_semseg import _loader
        was_training = self.model.training
        self.model.eval()
        self.evaluator.reset()
        n = len(dataset)
        bs = int(samples_per_gpu)
        batches = [[(i, 0) for i in range(s, min(s + bs, n))] for s in range(0, n, bs)]
        for keys, (events, offsets, labels, draws) in zip(batches, _loader(dataset, batches, min(workers, len(batches)))):
            pred = self.predict(events, offsets, draws, labels=labels)
            if on_batch is not None:
                on_batch([i for i, _ in keys], pred)
        m = self.evaluator.compute()
        self.model.train(was_training)
        iou = [float(v) for v in m["IoU"]]
        return {"aAcc": m["aAcc"], "mIoU": m["mIoU"], "mAcc": m["mAcc"],
                "IoU": {c: (None if math.isnan(v) else v) for c, v in zip(dataset.CLASSES, iou)}}
