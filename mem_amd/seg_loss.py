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

Out of scope: class weights, OHEM sampling, more than 32 classes.  No CPU fallback: CPU tensors raise.
"""
import torch

from . import ops
from ._lib import MemhipError


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
        mod.last_stats = dict(n_valid=stats[0], n_correct=stats[1], n_bad=stats[2])
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
    ``check_labels`` is set, which reads ``n_bad`` and raises on a bad label."""

    def __init__(self, ignore_index=255, align_corners=False, loss_weight=1.0, avg_non_ignore=False, check_labels=False):
        super().__init__()
        self.ignore_index = ignore_index
        self.align_corners = bool(align_corners)
        self.loss_weight = float(loss_weight)
        self.avg_non_ignore = bool(avg_non_ignore)
        self.check_labels = bool(check_labels)
        self.last_stats = None
        self._ws = None

    def _workspace(self, logits, labels):
        B, C, h, w = logits.shape
        need = int(ops.seg_plan(B, C, h, w, labels.shape[1], labels.shape[2], self.align_corners).ws_bytes)
        if self._ws is None or self._ws.numel() < need or self._ws.device != logits.device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=logits.device)
        return self._ws

    def forward(self, seg_logit, seg_label):
        seg_logit = _check_inputs(seg_logit, seg_label)
        loss = _SegCEFunction.apply(self, seg_logit, _labels_u8(seg_label))
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
