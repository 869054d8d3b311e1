"""The end of a segmentation decode head on the HIP path: the loss the reference trains with and the metrics it reports.

Both heads of the reference (``UPerHead`` and the auxiliary ``FCNHead``, ``align_corners=False``, ``CrossEntropyLoss`` at
weights 1.0 and 0.4: mem/semantic_segmentation/configs/_base_/models/upernet_beit.py:25-50) finish alike in mmseg 0.30::

    seg_logit = resize(seg_logit, size=seg_label.shape[2:], mode='bilinear', align_corners=False)
    loss      = cross_entropy(seg_logit, seg_label.squeeze(1), ignore_index=255)       # mean over ALL pixels
    acc_seg   = accuracy(seg_logit, seg_label, ignore_index=255)

and at test time ``resize -> softmax -> argmax -> intersect_and_union -> mIoU / mAcc / aAcc``.  ``SegCrossEntropy`` and
``SegEvaluator`` compute the same from the head's low-resolution logits with the kernels of csrc/seg_loss.hip: the resized
``[B, C, H, W]`` tensor is never written, loss + counts + gradient are one kernel, and the result is bit-reproducible (no float
atomics).  They take the logits of any head, torch or HIP, in any strides: NCHW as a torch head gives them, or the
``[B h w, ld]`` pixel rows of a GEMM head viewed as ``rows.view(B, h, w, ld)[..., :C].permute(0, 3, 1, 2)``.

Class weights and OHEM pixel sampling (mmseg's ``CrossEntropyLoss(class_weight=...)`` and ``OHEMPixelSampler``) live inside the
same fused kernel.  With ``z_p`` the resized logits of output pixel ``p``, ``l_p`` its label, ``nll_p = logsumexp(z_p) -
z_p[l_p]``, ``cw`` the class weights (default: ones) and ``s_p`` in {0, 1} the sampler's pixel weight::

    loss = loss_weight / N * sum over valid p of cw[l_p] * s_p * nll_p         N = B H W, or max(n_valid, 1) with avg_non_ignore

``N``, ``n_valid``, ``n_correct`` and ``acc_seg()`` depend on neither ``cw`` nor ``s`` (mmseg does not divide by the sum of the
weights, unlike torch's ``'mean'``).  The sampler is not differentiated through.  With ``n`` valid pixels and ``K = min_kept * B``:

* ``OHEMPixelSampler(thresh=T, min_kept=m)``: key ``k_p = softmax(z_p)[l_p]``; ``n == 0`` keeps nothing; else with the keys
  ascending ``a_0 <= ..``, ``t = max(a_min(K, n-1), T)`` and ``s_p = [k_p < t]``.
* ``OHEMPixelSampler(thresh=None, min_kept=m)``, top-k: key ``k_p = cw[l_p] * nll_p``; ``K' = min(K, n)``; ``K' == 0`` keeps
  nothing; else with the keys descending ``b_0 >= ..``, ``v = b_K'-1`` and ``s_p = [k_p >= v]``.  EVERY key equal to ``v`` is kept:
  mmseg keeps exactly ``K`` by whatever order its sort leaves among ties; here the result does not depend on a sort's order.

The hip arm computes the keys once in fp32, stores them as a ``[B, H, W]`` map (4 bytes per output pixel, 1 / C of the tensor
that is never written), finds the threshold with an exact radix select on the device (no sort, no host read) and takes every
keep decision on the stored keys.  ``impl="torch"`` is the readable restatement on plain torch ops (``F.interpolate``,
``log_softmax``, ``torch.sort``), on any device and dtype; it is what the tests hold the kernels against.

Out of scope: more than 32 classes, ``use_sigmoid`` and other loss types, a sampler across ranks (``K`` is per process, as in
mmseg).  ``impl="hip"`` has no CPU fallback: CPU tensors raise.
"""
import math

import torch
import torch.nn.functional as F

from . import ops
from ._lib import MemhipError


class OHEMPixelSampler:
    """mmseg's ``OHEMPixelSampler(thresh=None, min_kept=100000)``: a holder of the two numbers.  ``thresh`` in (0, 1]: pixels
    whose probability of the label is below ``max(thresh, the min_kept * B-th smallest)`` are kept; ``thresh=None``: the
    ``min_kept * B`` pixels of the largest loss (and every pixel that ties with the last of them)."""

    def __init__(self, thresh=None, min_kept=100000):
        if thresh is not None and not (isinstance(thresh, (int, float)) and 0.0 < float(thresh) <= 1.0):
            raise ValueError(f"OHEMPixelSampler: thresh must lie in (0, 1] or be None, got {thresh!r}")
        if isinstance(min_kept, bool) or int(min_kept) != min_kept or min_kept < 0:
            raise ValueError(f"OHEMPixelSampler: min_kept must be an integer >= 0, got {min_kept!r}")
        self.thresh = None if thresh is None else float(thresh)
        self.min_kept = int(min_kept)

    @property
    def mode(self):
        """the library's sampler number: 1 thresh, 2 top-k"""
        return ops.SEG_SAMPLER_TOPK if self.thresh is None else ops.SEG_SAMPLER_THRESH

    def __repr__(self):
        return f"OHEMPixelSampler(thresh={self.thresh!r}, min_kept={self.min_kept!r})"


def make_sampler(sampler):
    """None, an ``OHEMPixelSampler``, or mmseg's ``dict(type='OHEMPixelSampler', thresh=..., min_kept=...)``"""
    if sampler is None or isinstance(sampler, OHEMPixelSampler):
        return sampler
    if isinstance(sampler, dict):
        cfg = dict(sampler)
        kind = cfg.pop("type", None)
        if kind != "OHEMPixelSampler":
            raise NotImplementedError(f"sampler: type={kind!r}; OHEMPixelSampler is the pixel sampler of mem_amd.seg_loss")
        extra = set(cfg) - {"thresh", "min_kept"}
        if extra:
            raise TypeError(f"sampler: unsupported keys {sorted(extra)}")
        return OHEMPixelSampler(**cfg)
    raise TypeError(f"sampler: an OHEMPixelSampler, mmseg's dict or None, got {type(sampler).__name__}")


def make_class_weight(class_weight):
    """None, or a sequence / tensor of finite weights >= 0 -> a float32 CPU tensor [C]"""
    if class_weight is None:
        return None
    cw = torch.as_tensor(class_weight).detach().to("cpu", torch.float32).reshape(-1).clone()
    if cw.numel() == 0 or not bool(torch.isfinite(cw).all()) or bool((cw < 0).any()):
        raise ValueError("class_weight: a non-empty sequence of finite weights >= 0")
    return cw


def torch_seg_ce(seg_logit, seg_label, ignore_index=255, align_corners=False, loss_weight=1.0, avg_non_ignore=False,
                 class_weight=None, sampler=None, keep=None):
    """The definition on plain torch ops, any device and dtype: ``(loss, stats)`` with ``stats`` = n_valid, n_correct, n_bad,
    n_kept, threshold (tensors) and ``keep``, the sampler's mask ``[B, H, W]``.  ``seg_label``: integer ``[B, H, W]``.  ``keep``
    given: that mask stands in for the sampler's (tests hand one arm's mask to another)."""
    C_ = seg_logit.shape[1]
    lab = seg_label.long()
    up = F.interpolate(seg_logit, size=tuple(lab.shape[1:]), mode="bilinear", align_corners=align_corners)
    counted = torch.ones_like(lab, dtype=torch.bool) if ignore_index is None else lab != ignore_index
    valid = counted & (lab >= 0) & (lab < C_)
    tgt = torch.where(valid, lab, torch.zeros_like(lab))
    nll = -F.log_softmax(up, dim=1).gather(1, tgt[:, None])[:, 0]
    cwl = torch.ones_like(nll) if class_weight is None else class_weight.to(nll)[tgt]
    threshold = torch.full((), float("nan"), dtype=up.dtype, device=up.device)
    if keep is None:
        keep = valid
        if sampler is not None:
            with torch.no_grad():
                n, K = int(valid.sum()), sampler.min_kept * lab.shape[0]
                if sampler.thresh is not None:
                    key = F.softmax(up, dim=1).gather(1, tgt[:, None])[:, 0]
                    threshold = torch.full_like(threshold, -math.inf)
                    if n > 0:
                        a = torch.sort(key[valid]).values
                        threshold = torch.clamp(a[min(K, n - 1)], min=sampler.thresh)
                    keep = valid & (key < threshold)
                else:
                    key = cwl * nll
                    threshold = torch.full_like(threshold, math.inf)
                    if min(K, n) > 0:
                        threshold = torch.sort(key[valid], descending=True).values[min(K, n) - 1]
                    keep = valid & (key >= threshold)
    else:
        keep = keep.to(valid.device) & valid
    n_valid = valid.sum()
    N = n_valid.clamp(min=1).to(up.dtype) if avg_non_ignore else float(lab.numel())
    loss = (torch.where(keep, cwl * nll, torch.zeros_like(nll))).sum() * loss_weight / N
    stats = dict(n_valid=n_valid, n_correct=((up.argmax(1) == lab) & valid).sum(), n_bad=(counted & ~valid).sum(),
                 n_kept=keep.sum(), threshold=threshold, keep=keep)
    return loss, stats


def _labels_u8(seg_label):
    """uint8 [B, H, W] from uint8 [B, H, W] or mmseg's int64 [B, 1, H, W] / [B, H, W], converted once.  A value outside
    0..255 becomes 255: ignored under the default ignore_index, a bad label otherwise."""
    if seg_label.dim() == 4:
        assert seg_label.shape[1] == 1, "seg_label: [B, 1, H, W] or [B, H, W]"
        seg_label = seg_label[:, 0]
    assert seg_label.dim() == 3, "seg_label: [B, 1, H, W] or [B, H, W]"
    if seg_label.dtype != torch.uint8:
        assert not seg_label.dtype.is_floating_point, "seg_label: an integer tensor"
        seg_label = torch.where((seg_label < 0) | (seg_label > 255), 255, seg_label).to(torch.uint8)
    return seg_label.contiguous()


def _check_inputs(seg_logit, seg_label):
    if not (seg_logit.is_cuda and seg_label.is_cuda):
        raise MemhipError("mem_amd.seg_loss runs on the GPU only: seg_logit and seg_label must be CUDA tensors (no CPU fallback)")
    assert seg_logit.dim() == 4, "seg_logit: [B, C, h, w]"
    return seg_logit if seg_logit.dtype == torch.float32 else seg_logit.float()


class _SegCEFunction(torch.autograd.Function):
    """(loss-owning module, logits [B, C, h, w], labels u8 [B, H, W]) -> loss, a scalar; the gradient is the dz the forward
    kernel left, times grad_out * loss_weight / N (a device scalar the finish kernel wrote)."""

    @staticmethod
    def forward(ctx, mod, logits, labels):
        dz = torch.empty_like(logits)                 # the logits' strides when they are dense, contiguous otherwise
        out = torch.empty(3, dtype=torch.float32, device=logits.device)
        stats = torch.empty(3, dtype=torch.int64, device=logits.device)
        ops.seg_ce(logits, labels, dz, out, stats, mod._workspace(logits, labels), mod.ignore_index, mod.align_corners,
                   mod.avg_non_ignore, mod.loss_weight)
        mod.last_stats = dict(n_valid=stats[0], n_correct=stats[1], n_bad=stats[2], n_kept=stats[0], threshold=None)
        ctx.save_for_backward(dz, out)
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        dz, out = ctx.saved_tensors
        return None, dz * (grad_out * out[1]), None


class _SegCEWFunction(torch.autograd.Function):
    """``_SegCEFunction`` with class weights and / or a sampler: keys -> selection -> the weighted training kernel, all on the
    current stream.  ``out`` is f32 [4]: the three numbers of the loss and, behind them, the sampler's threshold."""

    @staticmethod
    def forward(ctx, mod, logits, labels):
        dz = torch.empty_like(logits)
        out = torch.empty(4, dtype=torch.float32, device=logits.device)
        stats = torch.empty(4, dtype=torch.int64, device=logits.device)
        ws = mod._workspace(logits, labels)
        cw = mod._class_weight(logits)
        smp, mode, keys, thr = mod.sampler, 0, None, None
        if smp is not None:
            mode, keys, thr = smp.mode, mod._keys(labels), out[3:]
            ops.seg_ohem_keys(logits, labels, keys, thr, mode, cw, mod.ignore_index, mod.align_corners)
            ops.seg_ohem_select(keys, thr, stats, ws, mode, smp.thresh, smp.min_kept, tuple(logits.shape[1:]))
        ops.seg_ce_w(logits, labels, dz, out, stats, ws, mod.ignore_index, mod.align_corners, mod.avg_non_ignore, mod.loss_weight,
                     cw, mode, keys, thr)
        mod.last_stats = dict(n_valid=stats[0], n_correct=stats[1], n_bad=stats[2], n_kept=stats[3],
                              threshold=out[3] if smp is not None else None)
        ctx.save_for_backward(dz, out)
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        dz, out = ctx.saved_tensors
        return None, dz * (grad_out * out[1]), None


class SegCrossEntropy(torch.nn.Module):
    """``module(seg_logit, seg_label) -> loss``: bilinear resize of ``seg_logit`` f32 ``[B, C, h, w]`` to the label's size
    and mmseg's ``CrossEntropyLoss(use_sigmoid=False, loss_weight=...)`` with ``ignore_index``, fused.

    ``loss = loss_weight * sum / N`` with ``N = B H W`` (mmseg 0.30's default) or ``max(n_valid, 1)`` with
    ``avg_non_ignore``; all labels ignored gives 0 with a zero gradient.  ``seg_label``: uint8 ``[B, H, W]``, or int64
    ``[B, 1, H, W]`` / ``[B, H, W]``.  ``last_stats`` holds the device scalars ``n_valid``, ``n_correct`` (argmax of the resized
    logits == label, ties to the lowest class) and ``n_bad`` (labels >= C that are not ``ignore_index``; they are treated as
    ignored) of the last call; ``acc_seg()`` is mmseg's accuracy in percent.  Nothing synchronises with the host unless
    ``check_labels`` is set, which reads ``n_bad`` and raises on a bad label.

    ``class_weight``: a sequence or tensor of ``C`` finite weights >= 0 (checked against ``C`` at the first call; kept as a
    non-persistent buffer, so ``.to()`` moves it and no state dict holds it).  ``sampler``: an ``OHEMPixelSampler`` or mmseg's
    ``dict(type='OHEMPixelSampler', thresh=..., min_kept=...)``; see the module's text for what it keeps.  With either,
    ``last_stats`` also holds ``n_kept`` (the pixels with ``s_p = 1``; ``n_valid`` without a sampler) and ``threshold`` (the
    sampler's device scalar, None without one); with neither, the module calls ``memhip_seg_ce`` exactly as before and
    ``n_kept`` is ``n_valid``.  The keys live in a buffer per label shape beside the workspace: a steady-state call allocates
    what the plain loss allocates.  ``impl="torch"``: the same definition on plain torch ops (``torch_seg_ce``), any device."""

    def __init__(self, ignore_index=255, align_corners=False, loss_weight=1.0, avg_non_ignore=False, check_labels=False,
                 class_weight=None, sampler=None, impl="hip"):
        super().__init__()
        if impl not in ("hip", "torch"):
            raise ValueError(f'impl: "hip" or "torch", got {impl!r}')
        self.ignore_index = ignore_index
        self.align_corners = bool(align_corners)
        self.loss_weight = float(loss_weight)
        self.avg_non_ignore = bool(avg_non_ignore)
        self.check_labels = bool(check_labels)
        self.sampler = make_sampler(sampler)
        self.impl = impl
        self.register_buffer("class_weight", make_class_weight(class_weight), persistent=False)
        self.last_stats = None
        self._ws = None
        self._key_bufs = {}

    def _workspace(self, logits, labels):
        B, C, h, w = logits.shape
        if self.class_weight is None and self.sampler is None:
            need = int(ops.seg_plan(B, C, h, w, labels.shape[1], labels.shape[2], self.align_corners).ws_bytes)
        else:
            smp = self.sampler
            need = int(ops.seg_ohem_plan(B, C, h, w, labels.shape[1], labels.shape[2], self.align_corners,
                                         0 if smp is None else smp.mode, None if smp is None else smp.thresh,
                                         0 if smp is None else smp.min_kept).ws_bytes)
        if self._ws is None or self._ws.numel() < need or self._ws.device != logits.device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=logits.device)
        return self._ws

    def _class_weight(self, logits):
        """the weights on the logits' device, checked against C"""
        cw = self.class_weight
        if cw is None:
            return None
        if cw.numel() != logits.shape[1]:
            raise ValueError("class_weight holds %d weights for logits of %d classes" % (cw.numel(), logits.shape[1]))
        if cw.device != logits.device or (self.impl == "hip" and cw.dtype != torch.float32):
            # once; .to() on the module does the same (the kernels read fp32 weights)
            cw = self.class_weight = cw.to(logits.device, torch.float32 if self.impl == "hip" else cw.dtype)
        return cw

    def _keys(self, labels):
        key = (tuple(labels.shape), str(labels.device))
        buf = self._key_bufs.get(key)
        if buf is None:
            buf = self._key_bufs[key] = torch.empty(tuple(labels.shape), dtype=torch.float32, device=labels.device)
        return buf

    def _torch_forward(self, seg_logit, seg_label):
        if seg_label.dim() == 4:
            assert seg_label.shape[1] == 1, "seg_label: [B, 1, H, W] or [B, H, W]"
            seg_label = seg_label[:, 0]
        seg_label = seg_label.long()
        seg_label = torch.where((seg_label < 0) | (seg_label > 255), 255, seg_label)      # as _labels_u8 reads them
        cw = self._class_weight(seg_logit)
        loss, stats = torch_seg_ce(seg_logit, seg_label.to(seg_logit.device), self.ignore_index, self.align_corners, self.loss_weight,
                                   self.avg_non_ignore, cw, self.sampler)
        if self.sampler is None:
            stats["threshold"] = None
        self.last_stats = stats
        return loss

    def forward(self, seg_logit, seg_label):
        if self.impl == "torch":
            loss = self._torch_forward(seg_logit, seg_label)
        else:
            seg_logit = _check_inputs(seg_logit, seg_label)
            fn = _SegCEFunction if self.class_weight is None and self.sampler is None else _SegCEWFunction
            loss = fn.apply(self, seg_logit, _labels_u8(seg_label))
        if self.check_labels:
            n_bad = int(self.last_stats["n_bad"])
            if n_bad:
                raise MemhipError("seg_label holds %d labels >= %d that are not ignore_index=%r" %
                                  (n_bad, seg_logit.shape[1], self.ignore_index))
        return loss

    def acc_seg(self):
        """mmseg's ``accuracy`` of the last call: 100 * n_correct / max(n_valid, 1), a device tensor."""
        s = self.last_stats
        return 100.0 * s["n_correct"].double() / s["n_valid"].clamp(min=1).double()


def all_reduce_sum(matrix):
    """Sum the confusion matrix over the ranks when torch.distributed runs with more than one (``--dist_eval``-style
    sharding of the validation set).  ``SegEvaluator.reduce`` holds this function; a test replaces it."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(matrix)
    return matrix


def metrics_from_confusion(matrix):
    """mmseg's ``eval_metrics(['mIoU'])`` from a confusion matrix (row = label, column = prediction), in float64: aAcc,
    mIoU, mAcc and the per-class IoU / Acc.  A class without a label and without a prediction has IoU NaN, one without a
    label Acc NaN; ``nanmean`` leaves them out."""
    m = matrix.detach().to("cpu", torch.float64)
    inter = m.diag()
    label = m.sum(1)
    pred = m.sum(0)
    iou = inter / (label + pred - inter)               # 0 / 0 = NaN: the class is absent
    acc = inter / label
    return dict(aAcc=float(inter.sum() / label.sum()), mIoU=float(torch.nanmean(iou)), mAcc=float(torch.nanmean(acc)),
                IoU=iou, Acc=acc)


class SegEvaluator:
    """Whole-image evaluation (``test_cfg.mode='whole'``): ``update(seg_logit, seg_label)`` adds the batch to an int64
    ``[C, C]`` confusion matrix on the device (resize -> argmax; softmax does not change an argmax), ``compute()`` derives
    the metrics, ``reset()`` clears, ``merge(other)`` adds another evaluator's matrix and ``compute(reduce=True)`` sums over
    the ranks first."""

    def __init__(self, num_classes, ignore_index=255, align_corners=False):
        assert 2 <= num_classes <= 32, "2 <= num_classes <= 32"
        self.num_classes = num_classes
        self.ignore_index = ignore_index
        self.align_corners = bool(align_corners)
        self.reduce = all_reduce_sum
        self.matrix = None

    def _matrix(self, device):
        if self.matrix is None:
            self.matrix = torch.zeros((self.num_classes, self.num_classes), dtype=torch.int64, device=device)
        return self.matrix

    def reset(self):
        if self.matrix is not None:
            self.matrix.zero_()

    @torch.no_grad()
    def update(self, seg_logit, seg_label):
        seg_logit = _check_inputs(seg_logit, seg_label)
        assert seg_logit.shape[1] == self.num_classes, (tuple(seg_logit.shape), self.num_classes)
        ops.seg_confusion(seg_logit, _labels_u8(seg_label), self._matrix(seg_logit.device), self.ignore_index,
                          self.align_corners)

    def merge(self, other):
        assert other.num_classes == self.num_classes
        if other.matrix is not None:
            mine = self._matrix(other.matrix.device)
            mine.add_(other.matrix.to(mine.device))
        return self

    def compute(self, reduce=False):
        assert self.matrix is not None, "SegEvaluator.compute() before any update(), merge() or matrix"
        return metrics_from_confusion(self.reduce(self.matrix.clone()) if reduce else self.matrix)
