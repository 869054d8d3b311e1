"""Finetuning criteria on the HIP loss kernel -- timm.loss.SoftTargetCrossEntropy and LabelSmoothingCrossEntropy, the two
non-default arms of the reference's three-way choice (mem/run_class_finetuning.py:609-616), restated from timm's published
definitions.  Both are one ``autograd.Function`` over ``memhip_ce_soft`` (include/memhip.h): the forward launch computes
the mean loss, the top-1 accuracy AND d(loss)/d(logits) (grad_scale 1/M) for bf16 or fp32 logits of any class count >= 2;
backward multiplies the kept gradient by the incoming scalar.  ``last_accuracy`` (a device scalar: top-1 against the hard
label, or against argmax of the soft target) spares a training loop its second pass over the logits."""
import torch
import torch.nn as nn

from . import ops


class _CeSoft(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, labels, smoothing, owner):
        assert logits.is_cuda and logits.dim() == 2, "loss kernels run on the GPU: logits [M, V] (no CPU fallback)"
        if logits.dtype not in (torch.bfloat16, torch.float32):
            raise TypeError(f"memhip_ce_soft takes bf16 or fp32 logits, got {logits.dtype}")
        x = logits if logits.stride(1) == 1 else logits.contiguous()
        M = x.shape[0]
        need_grad = ctx.needs_input_grad[0]
        dl = torch.empty_like(x, memory_format=torch.contiguous_format) if need_grad else None
        row_loss = torch.empty(M, dtype=torch.float32, device=x.device)
        row_correct = torch.empty(M, dtype=torch.int32, device=x.device)
        out2 = torch.empty(2, dtype=torch.float32, device=x.device)
        ops.ce_soft(x, row_loss, row_correct, out2, target=target, labels=labels, smoothing=smoothing, grad_scale=1.0 / M,
                    dlogits=dl)
        ctx.dl = dl
        owner.last_accuracy = out2[1]
        return out2[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        dl, ctx.dl = ctx.dl, None
        return dl * grad_out.to(dl.dtype), None, None, None, None


class SoftTargetCrossEntropy(nn.Module):
    """timm.loss.SoftTargetCrossEntropy: mean over the batch of sum_c(-target_c * log_softmax(x)_c); target [M, V] dense."""

    def __init__(self):
        super().__init__()
        self.last_accuracy = None

    def forward(self, x, target):
        assert target.shape == x.shape, "SoftTargetCrossEntropy: dense targets [M, V] (Mixup's output)"
        return _CeSoft.apply(x, target.to(torch.float32).contiguous(), None, 0.0, self)


class LabelSmoothingCrossEntropy(nn.Module):
    """timm.loss.LabelSmoothingCrossEntropy: (1 - smoothing) * nll + smoothing * mean_c(-log_softmax(x)_c), mean over the
    batch; hard labels [M] -- no dense target is built."""

    def __init__(self, smoothing=0.1):
        super().__init__()
        assert smoothing < 1.0
        self.smoothing = smoothing
        self.confidence = 1. - smoothing
        self.last_accuracy = None

    def forward(self, x, target):
        return _CeSoft.apply(x, None, target.to(torch.int64).contiguous(), float(self.smoothing), self)
