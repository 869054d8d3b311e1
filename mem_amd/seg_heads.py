"""Segmentation decode heads: mmseg 0.30's ``FCNHead`` -- the reference's auxiliary head
(mem/semantic_segmentation/configs/_base_/models/upernet_beit.py:38-50, configs/mem/upernet/mem_224_160k.py:64-77:
``in_index=2, channels=256, num_convs=1, concat_input=False, dropout_ratio=0.1``) -- and ``SegModel``, the thin
``EncoderDecoder`` that joins a backbone, a decode head and an optional auxiliary head::

    feat      = ReLU(SyncBN(Conv2d(in_channels, channels, 3, padding=1, bias=False)(inputs[in_index])))   # mmcv ConvModule
    seg_logit = Conv2d(channels, num_classes, 1)(Dropout2d(dropout_ratio)(feat))                           # cls_seg

``impl="torch"`` runs these layers as plain torch ops on any device and dtype (the reference arm of tests and benchmark).
``impl="hip"`` runs them on the library: the engine's fp32 map moves into the tokenizer's activation format (bf16
``[B, h+2, w+2, C]``, a zero ring), the 3x3 convolution, its data gradient and its weight gradient are the dVAE trainer's
kernels, and everything between the convolution and the loss is one pass each way (csrc/seg_head.hip): batch statistics,
then batch norm + ReLU + Dropout2d + classifier fused (the activation ``feat`` is never stored), and the backward split in
``sums`` and ``apply`` so that the SyncBN exchange (``reduce``) sits between them.  Both arms own the same parameters and
buffers under mmseg's keys, so a reference checkpoint's ``auxiliary_head.*`` loads with ``strict=True`` and moves freely
between the arms.

Precision of the hip arm: the placement torch's bf16 autocast would use.  Convolution operands bf16 with fp32 accumulation,
its output rounded to bf16 once; statistics, normalise -> affine -> ReLU -> dropout -> classifier in fp32 on fp32 parameters;
the gradient of the convolution's output rounded to bf16 once; logits, parameter gradients and the returned map gradient fp32.

Out of scope: ``UPerHead``, ``num_convs != 1``, ``concat_input``, dilation, class weights, OHEM samplers, more than 32 classes.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .seg_loss import SegCrossEntropy
from .syncbn import BufferCache, add_affine_grads, all_reduce_sum, backward_totals, batch_vectors


class ConvModule(nn.Module):
    """mmcv's ConvModule as the head uses it: ``conv`` (no bias) -> ``bn`` -> ReLU, under mmcv's attribute names."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, 3, padding=1, bias=False)
        self.bn = nn.BatchNorm2d(out_channels)


class _FCNHeadFunction(torch.autograd.Function):
    """The hip arm: fp32 map [B, Cin, h, w] -> logits, a [B, K, h, w] view of fp32 pixel rows.  The parameters are inputs so
    that a call under a frozen trunk still records; their gradients are accumulated into ``p.grad`` by the backward itself."""

    @staticmethod
    def forward(ctx, head, x, w, gamma, beta, wcls, bcls):
        ctx.head = head
        out, ctx.saved = head._hip_forward(x, keep=True)
        return out

    @staticmethod
    def backward(ctx, dlogit):
        return (None, ctx.head._hip_backward(ctx.saved, dlogit, ctx.needs_input_grad[1])) + (None,) * 5


class FCNHead(BufferCache, nn.Module):
    """mmseg 0.30 ``FCNHead(num_convs=1, concat_input=False)`` with its loss.

    ``forward(inputs)``: the backbone's tuple of maps -> logits ``[B, num_classes, h, w]`` from ``inputs[in_index]`` (the hip
    arm returns a strided view of pixel rows ``[B h w, num_classes]``, valid until this head's next call with that shape).
    ``forward_train(inputs, seg_label)`` -> ``{"loss_seg", "acc_seg"}`` (mmseg's ``losses``), ``forward_test(inputs)`` -> logits.

    The hip arm takes the engine's CUDA fp32 maps; ``in_channels`` and ``channels`` multiples of 64, ``channels <= 512``,
    ``2 <= num_classes <= 32``.  Everything runs on the current stream, nothing synchronises with the host; buffers are
    per shape and reused.  ``eval()`` uses the running statistics and drops nothing; under ``torch.no_grad()`` nothing is
    saved.  ``reduce`` is the SyncBN exchange (``all_reduce_sum``).  Dropout2d follows the mask contract of ``ops.Dropout``
    at site ``dropout_site``, row = sample, column = channel; the key of a training forward is ``drop_key`` when the caller
    sets one (a ``(key0, key1)`` per step, like the engine's), else ``(torch.initial_seed(), number of the call)``."""

    def __init__(self, in_channels=768, channels=256, num_classes=11, in_index=2, dropout_ratio=0.1, align_corners=False,
                 loss_weight=0.4, ignore_index=255, impl="hip", num_convs=1, concat_input=False, kernel_size=3, dilation=1,
                 class_weight=None, sampler=None, **kwargs):
        super().__init__()
        if num_convs != 1:
            raise NotImplementedError("num_convs: FCNHead mirrors num_convs=1 only (one conv + BN + ReLU block)")
        if concat_input:
            raise NotImplementedError("concat_input: FCNHead mirrors concat_input=False only")
        if kernel_size != 3:
            raise NotImplementedError("kernel_size: FCNHead mirrors the 3x3 convolution only")
        if dilation != 1:
            raise NotImplementedError("dilation: FCNHead mirrors dilation=1 only")
        if class_weight is not None:
            raise NotImplementedError("class_weight: class weights are not part of mem_amd.seg_loss")
        if sampler is not None:
            raise NotImplementedError("sampler: pixel samplers (OHEM) are not part of mem_amd.seg_loss")
        if kwargs:
            raise TypeError(f"FCNHead: unsupported arguments {sorted(kwargs)}")
        if impl not in ("hip", "torch"):
            raise ValueError(f'impl: "hip" or "torch", got {impl!r}')
        if not 0.0 <= dropout_ratio < 1.0:
            raise ValueError(f"dropout_ratio: 0 <= p < 1, got {dropout_ratio!r}")
        if impl == "hip":
            if in_channels % 64 or channels % 64 or channels > 512:
                raise ValueError(f"FCNHead(impl='hip'): in_channels={in_channels} and channels={channels} must be multiples of "
                                 "64 and channels <= 512")
            if not 2 <= num_classes <= 32:
                raise ValueError(f"FCNHead(impl='hip'): 2 <= num_classes <= 32, got {num_classes}")
        self.in_channels, self.channels, self.num_classes, self.in_index = in_channels, channels, num_classes, in_index
        self.dropout_ratio = float(dropout_ratio)
        self.align_corners = bool(align_corners)
        self.ignore_index = ignore_index
        self.impl = impl
        self.convs = nn.Sequential(ConvModule(in_channels, channels))
        self.conv_seg = nn.Conv2d(channels, num_classes, 1)
        nn.init.normal_(self.conv_seg.weight, mean=0.0, std=0.01)          # mmseg: normal_init(self.conv_seg, mean=0, std=0.01)
        nn.init.constant_(self.conv_seg.bias, 0.0)
        self.loss_decode = SegCrossEntropy(ignore_index=ignore_index, align_corners=align_corners, loss_weight=loss_weight)
        self.reduce = all_reduce_sum
        self.dropout_site = None             # ops.DROPOUT_SITE_HEAD (+ the head's number in a SegModel)
        self.drop_key = None
        self.keep_mask = None                # torch arm only: a [B, channels] 0/1 tensor in place of Dropout2d's own draw (tests)
        self._calls = 0
        self._bufs = {}
        self._w = None
        self._stamp = None

    # ------------------------------------------------------------------ the torch arm
    def _torch_forward(self, x):
        conv, bn = self.convs[0].conv, self.convs[0].bn
        y = F.conv2d(x, conv.weight, None, padding=1)
        if bn.training:
            with torch.no_grad():
                bn.num_batches_tracked += 1
        z = F.relu(F.batch_norm(y, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.training, bn.momentum, bn.eps))
        if self.training and self.dropout_ratio > 0.0:
            if self.keep_mask is not None:
                z = z * (self.keep_mask.to(z.dtype) / (1.0 - self.dropout_ratio))[:, :, None, None]
            else:
                z = F.dropout2d(z, self.dropout_ratio, True)
        return F.conv2d(z, self.conv_seg.weight, self.conv_seg.bias)

    # ------------------------------------------------------------------ the hip arm: buffers and weights
    def _buf_device(self):
        return self.conv_seg.weight.device

    def _weights(self):
        """(w16 [C, 9 Cin], wd16 [Cin, 9 C]): the bf16 operands of the forward and of the data gradient (the same kernel on
        the flipped, transposed weight), packed (ky, kx, c)-major.  Refreshed when the parameter has changed, never per forward."""
        from .vae_model import pack_conv_weight, pack_dgrad_weight
        w = self.convs[0].conv.weight
        stamp = (w._version, w.data_ptr())
        if self._w is None or stamp != self._stamp:
            wd = w.detach().float()
            self._w = (pack_conv_weight(wd).to(torch.bfloat16).contiguous(), pack_dgrad_weight("conv3", wd).to(torch.bfloat16).contiguous())
            self._stamp = stamp
        return self._w

    def refresh(self):
        """Drop the bf16 weight copies (a caller that changed the weight behind torch's version counter)."""
        self._stamp = None

    def _dropout(self):
        if not (self.training and self.dropout_ratio > 0.0):
            return None
        key = self.drop_key
        if key is None:
            key = (torch.initial_seed() & 0xFFFFFFFF, self._calls)
            self._calls += 1
        site = ops.DROPOUT_SITE_HEAD if self.dropout_site is None else self.dropout_site
        return ops.dropout_params(key[0], key[1], site, self.dropout_ratio)

    def _stats(self, Y, B, h, w):
        C = self.channels
        ws = self._buf("stats.ws", (ops.BN_GROUPS * 2 * C,), torch.float32)
        return ops.bn_stats_nhwc(Y, B, h, w, C, ws, None, True, out=self._buf("stats", (3, C), torch.float32))

    def _vectors(self):
        bn, cs = self.convs[0].bn, self.conv_seg
        return (bn.weight.detach().contiguous(), bn.bias.detach().contiguous(),
                cs.weight.detach().reshape(self.num_classes, self.channels), cs.bias.detach().contiguous())

    # ------------------------------------------------------------------ the hip arm: the two walks
    def _hip_forward(self, x, keep):
        B, Cin, h, w = x.shape
        C, K = self.channels, self.num_classes
        w16, _ = self._weights()
        Xp = ops.map_to_nhwc_pad(x, self._buf("xp", (B, h + 2, w + 2, Cin), zero=True))
        Y = self._buf("y", (B, h + 2, w + 2, C), zero=True)
        ops.conv2d_nhwc(Xp, w16, None, Y, B, h, w, Cin, C, 3, 1, 1)
        with torch.no_grad():
            # the convolution has no bias: the sums are unshifted
            mean, rstd, inv_n = batch_vectors(self.convs[0].bn, lambda: self._stats(Y, B, h, w), self.reduce)
            gamma, beta, wcls, bcls = self._vectors()
        d = self._dropout()
        rows = self._buf("logits", (B * h * w, K), torch.float32)
        ops.bnhead_fwd(Y, B, C, K, h, w, mean, rstd, gamma, beta, wcls, bcls, rows, dropout=d)
        out = rows.view(B, h, w, K).permute(0, 3, 1, 2).detach()       # a fresh tensor on the buffer
        return out, ((Xp, Y, mean, rstd, inv_n, d, (B, Cin, h, w)) if keep else None)

    def _hip_backward(self, saved, dlogit, need_dx):
        Xp, Y, mean, rstd, inv_n, d, (B, Cin, h, w) = saved
        C, K = self.channels, self.num_classes
        conv, bn, cs = self.convs[0].conv, self.convs[0].bn, self.conv_seg
        gamma, beta, wcls, _ = self._vectors()
        if dlogit.dtype != torch.float32:
            dlogit = dlogit.float()
        plan = ops.bnhead_plan(B, C, K, h, w)
        sums = self._buf("bwd.sums", (2, C), torch.float32)
        dwcls = self._buf("bwd.dwcls", (K, C), torch.float32)
        dbias = self._buf("bwd.dbias", (K,), torch.float32)
        ws = self._buf("bwd.ws", (int(plan.ws_bytes) // 4,), torch.float32)
        ops.bnhead_bwd_sums(dlogit, Y, B, C, K, h, w, mean, rstd, gamma, beta, wcls, sums, dwcls, dbias, ws, dropout=d)
        add_affine_grads(bn, sums)
        if cs.weight.requires_grad:
            self._grad(cs.weight).add_(dwcls.view(K, C, 1, 1))
        if cs.bias.requires_grad:
            self._grad(cs.bias).add_(dbias)
        tot = backward_totals(sums, inv_n, self.reduce)
        dY = ops.bnhead_bwd_apply(dlogit, Y, B, C, K, h, w, mean, rstd, gamma, beta, wcls, tot, 1.0,
                                  self._buf("dy", (B, h + 2, w + 2, C), zero=True), dropout=d)
        if conv.weight.requires_grad:
            need = ops.conv_wgrad_workspace(B, h, w, Cin, C, 3, 1, 1)
            wws = self._buf("wgrad.ws", (need,), torch.uint8) if need else None
            gw = self._buf("wgrad", (C, 9 * Cin), torch.float32)
            ops.conv_wgrad(dY, Xp, gw, B, h, w, Cin, C, 3, 1, 1, small_padded=True, accumulate=False, workspace=wws)
            self._grad(conv.weight).add_(gw.view(C, 3, 3, Cin).permute(0, 3, 1, 2))       # (ky, kx, c)-major -> [N, C, 3, 3]
        if not need_dx:
            return None
        dXp = self._buf("dxp", (B, h + 2, w + 2, Cin))
        ops.conv2d_nhwc(dY, self._weights()[1], None, dXp, B, h, w, C, Cin, 3, 1, 1)
        return ops.nhwc_pad_to_map(dXp, out=self._buf("dmap", (B, Cin, h, w), torch.float32)).detach()

    # ------------------------------------------------------------------ mmseg's interface
    def forward(self, inputs):
        x = inputs[self.in_index] if isinstance(inputs, (tuple, list)) else inputs
        if self.impl == "torch":
            return self._torch_forward(x)
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == self.in_channels):
            from ._lib import MemhipError
            raise MemhipError("FCNHead(impl='hip') takes the engine's CUDA fp32 map [B, %d, h, w] (no CPU fallback)" % self.in_channels)
        x = x.contiguous()
        conv, bn, cs = self.convs[0].conv, self.convs[0].bn, self.conv_seg
        params = [conv.weight, bn.weight, bn.bias, cs.weight, cs.bias]
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            return _FCNHeadFunction.apply(self, x, *params)
        return self._hip_forward(x.detach(), keep=False)[0]

    def forward_train(self, inputs, seg_label):
        seg_logit = self.forward(inputs)
        loss = self.loss_decode(seg_logit, seg_label)
        return {"loss_seg": loss, "acc_seg": self.loss_decode.acc_seg()}

    def forward_test(self, inputs):
        return self.forward(inputs)


class SegModel(nn.Module):
    """mmseg's ``EncoderDecoder``, thin: ``backbone`` (an ``EvBEiT``: images -> a tuple of maps), ``decode_head`` and an optional
    ``auxiliary_head`` (``FCNHead``s).  ``forward_train(img, seg_label)`` -> ``{"decode.loss_seg", "decode.acc_seg", "aux.loss_seg",
    "aux.acc_seg"}``; ``encode_decode(img)`` -> the decode head's logits at the head's resolution (``test_cfg.mode='whole'``:
    the resize to the label's size is ``SegEvaluator``'s).  One object for an optimizer and an evaluator."""

    def __init__(self, backbone, decode_head, auxiliary_head=None):
        super().__init__()
        self.backbone = backbone
        self.decode_head = decode_head
        self.auxiliary_head = auxiliary_head
        for i, head in enumerate(h for h in (decode_head, auxiliary_head) if h is not None):
            if getattr(head, "dropout_site", 0) is None:
                head.dropout_site = ops.DROPOUT_SITE_HEAD + i          # each head its own Dropout2d masks

    def extract_feat(self, img):
        return self.backbone(img)

    def forward_train(self, img, seg_label):
        feats = self.extract_feat(img)
        out = {"decode." + k: v for k, v in self.decode_head.forward_train(feats, seg_label).items()}
        if self.auxiliary_head is not None:
            out.update({"aux." + k: v for k, v in self.auxiliary_head.forward_train(feats, seg_label).items()})
        return out

    def encode_decode(self, img):
        return self.decode_head.forward_test(self.extract_feat(img))

    def forward(self, img):
        return self.encode_decode(img)
