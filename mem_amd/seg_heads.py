"""Segmentation decode heads: mmseg 0.30's ``FCNHead`` -- the reference's auxiliary head
(mem/semantic_segmentation/configs/_base_/models/upernet_beit.py:38-50, configs/mem/upernet/mem_224_160k.py:64-77:
``in_index=2, channels=256, num_convs=1, concat_input=False, dropout_ratio=0.1``) --, mmseg 0.30's ``PSPHead``
(mmseg/models/decode_heads/psp_head.py; its layers are ``UPerHead.psp_forward`` + ``cls_seg``, the pyramid branch of the
reference's decode head, upernet_beit.py:25-37: ``pool_scales=(1, 2, 3, 6), channels=512``), mmseg 0.30's ``UPerHead``
(mmseg/models/decode_heads/uper_head.py: that decode head itself, ``in_index=[0, 1, 2, 3]``) and ``SegModel``, the thin
``EncoderDecoder`` that joins a backbone, a decode head and an optional auxiliary head::

    FCNHead   feat = ReLU(SyncBN(Conv2d(in_channels, channels, 3, padding=1, bias=False)(inputs[in_index])))   # mmcv ConvModule
    PSPHead   outs = [resize(ReLU(SyncBN(Conv2d(in_channels, channels, 1, bias=False)(AdaptiveAvgPool2d(s)(x)))), size of x)
                      for s in pool_scales]                                                                    # PPM
              feat = ReLU(SyncBN(Conv2d(in_channels + len(pool_scales) channels, channels, 3, padding=1, bias=False)(
                         cat([x] + outs, dim=1))))                                                             # bottleneck
    UPerHead  lat_l = ReLU(SyncBN(Conv2d(in_channels[l], channels, 1, bias=False)(inputs[in_index[l]]))), l < L - 1; lat_L-1 = PSPHead's
              feat on the last level; top-down lat_l-1 += resize(lat_l); out_l = ReLU(SyncBN(Conv2d(channels, channels, 3, ..)(lat_l)));
              feat = ReLU(SyncBN(Conv2d(L channels, channels, 3, padding=1, bias=False)(cat([out_0] + [resize(out_l)], 1))))  # fpn_bottleneck
    all       seg_logit = Conv2d(channels, num_classes, 1)(Dropout2d(dropout_ratio)(feat))                     # cls_seg

``impl="torch"`` runs these layers as plain torch ops on any device and dtype (the reference arm of tests and benchmark).
``impl="hip"`` runs them on the library: the engine's fp32 map moves into the tokenizer's activation format (bf16
``[B, h+2, w+2, C]``, a zero ring), the convolutions, their data gradients and their weight gradients are the dVAE trainer's
kernels, and everything between the 3x3 convolution and the loss is one pass each way (csrc/seg_head.hip): batch statistics,
then batch norm + ReLU + Dropout2d + classifier fused (the activation ``feat`` is never stored), and the backward split in
``sums`` and ``apply`` so that the SyncBN exchange (``reduce``) sits between them.  That walk is one piece of code for both
heads (``_BnClsHead``).  ``PSPHead`` puts ``PyramidPooling`` in front of it (csrc/ppm.hip): all scales pooled in one pass over
the map, and batch norm + ReLU + bilinear resize + concat written straight as the bottleneck's operand -- the branch
activations, their upsampled maps and an fp32 concat are never stored.  ``UPerHead`` puts the FPN part between the two
(csrc/fpn.hip): the laterals and FPN convolutions are the library's, the top-down sums and ``fpn_bottleneck``'s operand are
written with batch norm + ReLU + resize fused, and the backward transposes both as ordered gathers.  Both arms own the same
parameters and buffers under mmseg's keys, so a reference checkpoint's ``auxiliary_head.*`` (``FCNHead``) and ``decode_head.*``
(``UPerHead``; its ``psp_modules.*`` / ``bottleneck.*`` entries: ``PSPHead``) load with ``strict=True`` and move freely between
the arms.

Precision of the hip arm: the placement torch's bf16 autocast would use.  Convolution operands bf16 with fp32 accumulation,
each convolution output rounded to bf16 once; pooling sums, statistics, normalise -> affine -> ReLU -> interpolation -> dropout
-> classifier in fp32 on fp32 parameters; a value is rounded to bf16 once where it becomes a convolution operand or the
gradient of a convolution's output; logits, parameter gradients and the returned map gradient fp32.

The loss: every head takes ``loss_decode=``, a ``SegCrossEntropy`` or mmseg's ``dict(type='CrossEntropyLoss', use_sigmoid=False,
loss_weight=..., class_weight=[...], avg_non_ignore=...)`` with this project's extra key ``sampler=dict(type='OHEMPixelSampler',
thresh=..., min_kept=...)`` (mmseg puts the sampler beside the loss in the head's config; here it belongs to the loss that
applies it).  The head builds ``self.loss_decode`` from it with its own ``ignore_index`` and ``align_corners``; a dict's loss runs
on the head's arm (``impl="torch"``: ``seg_loss.torch_seg_ce``, plain torch ops on any device).  A ``SegCrossEntropy`` instance is
used as it is, not copied: the head WRITES its own ``ignore_index`` and ``align_corners`` into the caller's object, and one instance given
to two heads is shared by them (one ``last_stats``, one workspace); give each head its own.  Without ``loss_decode=`` the loss is
the plain fused one at the head's ``loss_weight``, as before.  The head keywords ``class_weight=`` and ``sampler=`` still raise.

Out of scope: the mmseg runner, schedules and data pipeline, sliding-window test mode, ``num_convs != 1``, ``concat_input``,
dilation, ``use_sigmoid`` and other loss types, more than 32 classes, ``channels > 512``, more than 4 levels on the hip arm.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .seg_loss import SegCrossEntropy
from .syncbn import BufferCache, add_affine_grads, all_reduce_sum, backward_totals, batch_vectors, batch_vectors_stacked, grad_of


class ConvModule(nn.Module):
    """mmcv's ConvModule as the heads use it: ``conv`` (no bias) -> ``bn`` -> ReLU, under mmcv's attribute names."""

    def __init__(self, in_channels, out_channels, kernel_size=3):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, padding=kernel_size // 2, bias=False)
        self.bn = nn.BatchNorm2d(out_channels)


class _HeadFunction(torch.autograd.Function):
    """The hip arm: fp32 map [B, Cin, h, w] -> logits, a [B, K, h, w] view of fp32 pixel rows.  The parameters are inputs so
    that a call under a frozen trunk still records; their gradients are accumulated into ``p.grad`` by the backward itself."""

    @staticmethod
    def forward(ctx, head, x, *params):
        ctx.head, ctx.n_params = head, len(params)
        out, ctx.saved = head._hip_forward(x, keep=True)
        return out

    @staticmethod
    def backward(ctx, dlogit):
        return (None, ctx.head._hip_backward(ctx.saved, dlogit, ctx.needs_input_grad[1])) + (None,) * ctx.n_params


class _LevelsFunction(torch.autograd.Function):
    """``_HeadFunction`` for a head that reads several maps (``UPerHead``): ``n`` fp32 maps -> logits; the backward returns a
    gradient per map (None where nobody asked)."""

    @staticmethod
    def forward(ctx, head, n, *args):
        ctx.head, ctx.n, ctx.n_params = head, n, len(args) - n
        out, ctx.saved = head._hip_forward(args[:n], keep=True)
        return out

    @staticmethod
    def backward(ctx, dlogit):
        grads = ctx.head._hip_backward(ctx.saved, dlogit, ctx.needs_input_grad[2:2 + ctx.n])
        return (None, None) + tuple(grads) + (None,) * ctx.n_params


class _BnClsHead(BufferCache, nn.Module):
    """What the decode heads share: the walk from the padded bf16 operand of a head's last 3x3 ConvModule (``_cm()``) to the
    logits and back (``_tail_forward`` / ``_tail_backward``), the bf16 weight copies, Dropout2d's keys, and mmseg's interface."""

    _default_loss_weight = 1.0           # the constructor's default: what ``loss_weight=`` may be beside ``loss_decode=``

    def _init_tail(self, channels, num_classes, in_index, dropout_ratio, align_corners, loss_weight, ignore_index, impl,
                   loss_decode=None):
        self.channels, self.num_classes, self.in_index = channels, num_classes, in_index
        self.dropout_ratio = float(dropout_ratio)
        self.align_corners = bool(align_corners)
        self.ignore_index = ignore_index
        self.impl = impl
        self.conv_seg = nn.Conv2d(channels, num_classes, 1)
        nn.init.normal_(self.conv_seg.weight, mean=0.0, std=0.01)          # mmseg: normal_init(self.conv_seg, mean=0, std=0.01)
        nn.init.constant_(self.conv_seg.bias, 0.0)
        self.loss_decode = self._make_loss(loss_decode, loss_weight, ignore_index, align_corners, impl)
        self.reduce = all_reduce_sum
        self.dropout_site = None             # ops.DROPOUT_SITE_HEAD (+ the head's number in a SegModel)
        self.drop_key = None
        self.keep_mask = None                # torch arm only: a [B, channels] 0/1 tensor in place of Dropout2d's own draw (tests)
        self._calls = 0
        self._bufs = {}
        self._w = {}

    @classmethod
    def _make_loss(cls, loss_decode, loss_weight, ignore_index, align_corners, impl):
        """the head's ``SegCrossEntropy``: the plain one at ``loss_weight``, or what ``loss_decode=`` describes"""
        if loss_decode is None:
            return SegCrossEntropy(ignore_index=ignore_index, align_corners=align_corners, loss_weight=loss_weight)
        if loss_weight != cls._default_loss_weight:
            raise ValueError(f"{cls.__name__}: loss_decode= carries the loss weight; loss_weight={loss_weight!r} beside it is ambiguous")
        if isinstance(loss_decode, SegCrossEntropy):
            loss_decode.ignore_index, loss_decode.align_corners = ignore_index, bool(align_corners)
            return loss_decode
        if not isinstance(loss_decode, dict):
            raise TypeError(f"loss_decode: a SegCrossEntropy or mmseg's dict, got {type(loss_decode).__name__}")
        cfg = dict(loss_decode)
        kind = cfg.pop("type", "CrossEntropyLoss")
        if kind != "CrossEntropyLoss":
            raise NotImplementedError(f"loss_decode: type={kind!r}; CrossEntropyLoss is the loss of mem_amd.seg_loss")
        if cfg.pop("use_sigmoid", False):
            raise NotImplementedError("loss_decode: use_sigmoid=True (binary cross entropy) is not part of mem_amd.seg_loss")
        if cfg.pop("use_mask", False):
            raise NotImplementedError("loss_decode: use_mask=True is not part of mem_amd.seg_loss")
        if cfg.pop("reduction", "mean") != "mean":
            raise NotImplementedError("loss_decode: reduction='mean' only")
        cfg.pop("loss_name", None)
        extra = set(cfg) - {"loss_weight", "class_weight", "avg_non_ignore", "sampler", "check_labels", "impl"}
        if extra:
            raise TypeError(f"loss_decode: unsupported keys {sorted(extra)}")
        cfg.setdefault("impl", impl)
        return SegCrossEntropy(ignore_index=ignore_index, align_corners=align_corners, **cfg)

    @classmethod
    def _check_common(cls, impl, dropout_ratio, in_channels, channels, num_classes, class_weight, sampler, kwargs):
        name = cls.__name__
        if class_weight is not None:
            raise NotImplementedError("class_weight: the head takes class weights through loss_decode=dict(type='CrossEntropyLoss', "
                                      "class_weight=[...]), not as a keyword of its own")
        if sampler is not None:
            raise NotImplementedError("sampler: the head takes a pixel sampler (OHEM) through loss_decode=dict(type='CrossEntropyLoss', "
                                      "sampler=dict(type='OHEMPixelSampler', ...)), not as a keyword of its own")
        if kwargs:
            raise TypeError(f"{name}: unsupported arguments {sorted(kwargs)}")
        if impl not in ("hip", "torch"):
            raise ValueError(f'impl: "hip" or "torch", got {impl!r}')
        if not 0.0 <= dropout_ratio < 1.0:
            raise ValueError(f"dropout_ratio: 0 <= p < 1, got {dropout_ratio!r}")
        if impl == "hip":
            if in_channels % 64 or channels % 64 or channels > 512:
                raise ValueError(f"{name}(impl='hip'): in_channels={in_channels} and channels={channels} must be multiples of "
                                 "64 and channels <= 512")
            if not 2 <= num_classes <= 32:
                raise ValueError(f"{name}(impl='hip'): 2 <= num_classes <= 32, got {num_classes}")

    def _cm(self):
        """the ConvModule (3x3) in front of ``cls_seg``"""
        raise NotImplementedError

    def _params(self):
        """the parameters the hip arm's backward feeds, in a fixed order"""
        raise NotImplementedError

    # ------------------------------------------------------------------ the torch arm
    @staticmethod
    def _torch_cm(m, x):
        """a ``ConvModule`` on plain torch ops: conv -> batch norm (with its bookkeeping) -> ReLU"""
        y = F.conv2d(x, m.conv.weight, None, padding=m.conv.padding)
        bn = m.bn
        if bn.training:
            with torch.no_grad():
                bn.num_batches_tracked += 1
        return F.relu(F.batch_norm(y, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.training, bn.momentum, bn.eps))

    def _torch_tail(self, x):
        conv, bn = self._cm().conv, self._cm().bn
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

    def _packed(self, conv, kind):
        """(w16 [N, k k Cin], wd16 [Cin, k k N]) of ``conv`` ("conv3" / "conv1"): the bf16 operands of the forward and of the data
        gradient (the same kernel on the flipped, transposed weight), packed (ky, kx, c)-major.  Refreshed when the parameter
        has changed, never per forward."""
        from .vae_model import pack_conv_weight, pack_dgrad_weight
        w = conv.weight
        stamp = (w._version, w.data_ptr())
        got = self._w.get(id(conv))
        if got is None or got[0] != stamp:
            wd = w.detach().float()
            got = self._w[id(conv)] = (stamp, (pack_conv_weight(wd).to(torch.bfloat16).contiguous(),
                                               pack_dgrad_weight(kind, wd).to(torch.bfloat16).contiguous()))
        return got[1]

    def _weights(self):
        return self._packed(self._cm().conv, "conv3")

    def refresh(self):
        """Drop the bf16 weight copies (a caller that changed a weight behind torch's version counter)."""
        self._w = {}

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
        bn, cs = self._cm().bn, self.conv_seg
        return (bn.weight.detach().contiguous(), bn.bias.detach().contiguous(),
                cs.weight.detach().reshape(self.num_classes, self.channels), cs.bias.detach().contiguous())

    # ------------------------------------------------------------------ the hip arm: the shared walk
    def _tail_forward(self, Xp, B, Cin, h, w, keep):
        """Xp bf16 [B, h+2, w+2, Cin] -> (logits, what the backward needs)"""
        C, K = self.channels, self.num_classes
        w16, _ = self._weights()
        Y = self._buf("y", (B, h + 2, w + 2, C), zero=True)
        ops.conv2d_nhwc(Xp, w16, None, Y, B, h, w, Cin, C, 3, 1, 1)
        with torch.no_grad():
            # the convolution has no bias: the sums are unshifted
            mean, rstd, inv_n = batch_vectors(self._cm().bn, lambda: self._stats(Y, B, h, w), self.reduce)
            gamma, beta, wcls, bcls = self._vectors()
        d = self._dropout()
        rows = self._buf("logits", (B * h * w, K), torch.float32)
        ops.bnhead_fwd(Y, B, C, K, h, w, mean, rstd, gamma, beta, wcls, bcls, rows, dropout=d)
        out = rows.view(B, h, w, K).permute(0, 3, 1, 2).detach()       # a fresh tensor on the buffer
        return out, ((Xp, Y, mean, rstd, inv_n, d, (B, Cin, h, w)) if keep else None)

    def _tail_backward(self, saved, dlogit, need_dx):
        """dlogit [B, K, h, w] -> dXp bf16 [B, h+2, w+2, Cin] (interiors; None when nobody needs it); the gradients of the
        3x3 ConvModule and of ``conv_seg`` are added to ``p.grad``"""
        Xp, Y, mean, rstd, inv_n, d, (B, Cin, h, w) = saved
        C, K = self.channels, self.num_classes
        conv, bn, cs = self._cm().conv, self._cm().bn, self.conv_seg
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
        return dXp

    # ------------------------------------------------------------------ mmseg's interface
    def forward(self, inputs):
        x = inputs[self.in_index] if isinstance(inputs, (tuple, list)) else inputs
        if self.impl == "torch":
            return self._torch_forward(x)
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == self.in_channels):
            from ._lib import MemhipError
            raise MemhipError("%s(impl='hip') takes the engine's CUDA fp32 map [B, %d, h, w] (no CPU fallback)"
                              % (type(self).__name__, self.in_channels))
        x = x.contiguous()
        params = self._params()
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            return _HeadFunction.apply(self, x, *params)
        return self._hip_forward(x.detach(), keep=False)[0]

    def forward_train(self, inputs, seg_label):
        seg_logit = self.forward(inputs)
        loss = self.loss_decode(seg_logit, seg_label)
        return {"loss_seg": loss, "acc_seg": self.loss_decode.acc_seg()}

    def forward_test(self, inputs):
        return self.forward(inputs)


class FCNHead(_BnClsHead):
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

    _default_loss_weight = 0.4

    def __init__(self, in_channels=768, channels=256, num_classes=11, in_index=2, dropout_ratio=0.1, align_corners=False,
                 loss_weight=0.4, ignore_index=255, impl="hip", num_convs=1, concat_input=False, kernel_size=3, dilation=1,
                 class_weight=None, sampler=None, loss_decode=None, **kwargs):
        super().__init__()
        if num_convs != 1:
            raise NotImplementedError("num_convs: FCNHead mirrors num_convs=1 only (one conv + BN + ReLU block)")
        if concat_input:
            raise NotImplementedError("concat_input: FCNHead mirrors concat_input=False only")
        if kernel_size != 3:
            raise NotImplementedError("kernel_size: FCNHead mirrors the 3x3 convolution only")
        if dilation != 1:
            raise NotImplementedError("dilation: FCNHead mirrors dilation=1 only")
        self._check_common(impl, dropout_ratio, in_channels, channels, num_classes, class_weight, sampler, kwargs)
        self.in_channels = in_channels
        self.convs = nn.Sequential(ConvModule(in_channels, channels))
        self._init_tail(channels, num_classes, in_index, dropout_ratio, align_corners, loss_weight, ignore_index, impl, loss_decode)

    def _cm(self):
        return self.convs[0]

    def _params(self):
        conv, bn, cs = self.convs[0].conv, self.convs[0].bn, self.conv_seg
        return [conv.weight, bn.weight, bn.bias, cs.weight, cs.bias]

    def _torch_forward(self, x):
        return self._torch_tail(x)

    # ------------------------------------------------------------------ the hip arm: the movers around the shared walk
    def _hip_forward(self, x, keep):
        B, Cin, h, w = x.shape
        Xp = ops.map_to_nhwc_pad(x, self._buf("xp", (B, h + 2, w + 2, Cin), zero=True))
        return self._tail_forward(Xp, B, Cin, h, w, keep)

    def _hip_backward(self, saved, dlogit, need_dx):
        dXp = self._tail_backward(saved, dlogit, need_dx)
        if dXp is None:
            return None
        B, Cin, h, w = saved[-1]
        return ops.nhwc_pad_to_map(dXp, out=self._buf("dmap", (B, Cin, h, w), torch.float32)).detach()


class PyramidPooling:
    """The pyramid branch of ``PSPHead`` and of ``UPerHead`` on the hip path: fp32 map ``[B, Cin, h, w]`` -> the
    interior of ``Xcat`` bf16 ``[B, h+2, w+2, Cin + n C]`` (``forward``), and ``dXcat`` -> the fp32 map gradient (``backward``);
    who consumes ``Xcat`` is the caller's business.  ``modules``: the 1x1 ``ConvModule`` per pool scale; ``owner``: whose buffer
    cache (``_buf``, names under ``ppm.``), bf16 weight copies (``_packed``) and SyncBN hook (``reduce``) it uses.

    Per training step one ``reduce(., "stats")`` for the statistics of all scales ([n, 3, C]) and one ``reduce(., "bwd")`` for
    their backward sums ([n, 2, C])."""

    def __init__(self, owner, modules, pool_scales, in_channels, channels, align_corners=False):
        self.owner, self.modules, self.scales = owner, list(modules), tuple(int(s) for s in pool_scales)
        self.in_channels, self.channels, self.align_corners = in_channels, channels, bool(align_corners)

    def check(self, B, h, w, training):
        """refuse what the kernels' tables and torch's batch norm refuse, by name"""
        if min(h, w) < max(self.scales):
            raise ValueError("pool_scales=%r on a map of %dx%d: the hip arm resizes upwards only, min(h, w) >= max(pool_scales)"
                             % (self.scales, h, w))
        if training:
            import torch.distributed as dist
            alone = not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)
            for s in self.scales:
                if B * s * s == 1 and alone:
                    raise ValueError("Expected more than 1 value per channel when training: pool scale %d of a batch of %d gives "
                                     "its batch norm one value (torch's batch norm refuses it too)" % (s, B))

    def _stats(self, Y, B):
        C, o = self.channels, self.owner
        ws = o._buf("ppm.stats.ws", (ops.BN_GROUPS * 2 * C,), torch.float32)
        out = o._buf("ppm.stats", (len(self.scales), 3, C), torch.float32)
        for i, s in enumerate(self.scales):
            ops.bn_stats_nhwc(Y[i], B, s, s, C, ws, None, True, out=out[i])
        return out

    def forward(self, x, xcat, keep):
        B, Cin, h, w = x.shape
        C, o, sc = self.channels, self.owner, self.scales
        P = [o._buf("ppm.p%d" % i, (B, s + 2, s + 2, Cin), zero=True) for i, s in enumerate(sc)]
        ops.ppm_pool(x, sc, P)
        Y = [o._buf("ppm.y%d" % i, (B, s + 2, s + 2, C), zero=True) for i, s in enumerate(sc)]
        for i, s in enumerate(sc):
            ops.conv2d_nhwc(P[i], o._packed(self.modules[i].conv, "conv1")[0], None, Y[i], B, s, s, Cin, C, 1, 1, 0)
        with torch.no_grad():
            bns = [m.bn for m in self.modules]
            mean, rstd, inv_n = batch_vectors_stacked(bns, lambda: self._stats(Y, B), o.reduce)
            gamma, beta = torch.stack([bn.weight.detach() for bn in bns]), torch.stack([bn.bias.detach() for bn in bns])
        ops.ppm_concat_fwd(x, sc, Y, mean, rstd, gamma, beta, xcat, self.align_corners)
        return (P, Y, mean, rstd, gamma, beta, inv_n, (B, Cin, h, w)) if keep else None

    def backward(self, saved, dxcat, need_dx):
        P, Y, mean, rstd, gamma, beta, inv_n, (B, Cin, h, w) = saved
        C, o, sc = self.channels, self.owner, self.scales
        n = len(sc)
        g = [o._buf("ppm.g%d" % i, (B * s * s, C), torch.float32) for i, s in enumerate(sc)]
        sums = o._buf("ppm.sums", (n, 2, C), torch.float32)
        ops.ppm_concat_bwd_sums(dxcat, Cin, sc, Y, mean, rstd, gamma, beta, g, sums, self.align_corners)
        for i, m in enumerate(self.modules):
            add_affine_grads(m.bn, sums[i])
        # the sums of every rank, divided on the device by the counts the forward's statistics had; eval statistics: none
        tot = None if inv_n is None else (o.reduce(sums.clone(), "bwd") * inv_n[:, None, :]).contiguous()
        dY = [o._buf("ppm.dy%d" % i, (B, s + 2, s + 2, C), zero=True) for i, s in enumerate(sc)]
        ops.ppm_bwd_apply(g, sc, Y, mean, rstd, gamma, beta, tot, [1.0] * n, dY, (h, w))
        for i, (s, m) in enumerate(zip(sc, self.modules)):
            if m.conv.weight.requires_grad:
                need = ops.conv_wgrad_workspace(B, s, s, Cin, C, 1, 1, 0)
                wws = o._buf("ppm.wgrad.ws", (need,), torch.uint8) if need else None
                gw = o._buf("ppm.wgrad", (C, Cin), torch.float32)
                ops.conv_wgrad(dY[i], P[i], gw, B, s, s, Cin, C, 1, 1, 0, small_padded=True, accumulate=False, workspace=wws)
                grad_of(m.conv.weight).add_(gw.view(C, Cin, 1, 1))
        if not need_dx:
            return None
        dP = [o._buf("ppm.dp%d" % i, (B, s + 2, s + 2, Cin)) for i, s in enumerate(sc)]
        for i, s in enumerate(sc):
            ops.conv2d_nhwc(dY[i], o._packed(self.modules[i].conv, "conv1")[1], None, dP[i], B, s, s, C, Cin, 1, 1, 0)
        return ops.ppm_dmap(dxcat, Cin, sc, dP, o._buf("ppm.dmap", (B, Cin, h, w), torch.float32)).detach()


class PSPHead(_BnClsHead):
    """mmseg 0.30 ``PSPHead`` (mmseg/models/decode_heads/psp_head.py) with its loss: pyramid pooling at ``pool_scales``, a 1x1
    ConvModule per scale, bilinear resize back, concat with the input, a 3x3 bottleneck ConvModule, ``cls_seg`` -- the
    layers, and under ``psp_modules.{i}.1.*`` / ``bottleneck.*`` the state-dict keys and shapes, of ``UPerHead.psp_forward`` in the
    reference's decode head (mem/semantic_segmentation/configs/_base_/models/upernet_beit.py:25-37).

    The interface, the hip arm's inputs and limits, Dropout2d's keys and ``reduce`` are ``FCNHead``'s.  In addition the hip
    arm takes at most 4 pool scales, each ``1 <= s <= 8``, and maps with ``min(h, w) >= max(pool_scales)`` (7x7 at 224^2, 14x20
    at 440x640); a training call in which a scale's batch norm would see one value (``B s^2 == 1``, no process group) is refused
    as torch's batch norm refuses it.  ``reduce`` is called with the tags "stats", "stats" (pyramid, bottleneck) in a training
    forward and "bwd", "bwd" (bottleneck, pyramid) in its backward."""

    def __init__(self, in_channels=768, channels=512, num_classes=11, in_index=3, pool_scales=(1, 2, 3, 6), dropout_ratio=0.1,
                 align_corners=False, loss_weight=1.0, ignore_index=255, impl="hip", class_weight=None, sampler=None, loss_decode=None,
                 **kwargs):
        super().__init__()
        self._check_common(impl, dropout_ratio, in_channels, channels, num_classes, class_weight, sampler, kwargs)
        pool_scales = tuple(pool_scales)
        if not pool_scales or any(int(s) != s or s < 1 for s in pool_scales):
            raise ValueError(f"pool_scales: positive integers, got {pool_scales!r}")
        if impl == "hip":
            if len(pool_scales) > ops.PPM_MAX_SCALES:
                raise ValueError(f"PSPHead(impl='hip'): at most {ops.PPM_MAX_SCALES} pool_scales, got {pool_scales!r}")
            if any(not 1 <= s <= ops.PPM_MAX_SCALE for s in pool_scales):
                raise ValueError(f"PSPHead(impl='hip'): 1 <= s <= {ops.PPM_MAX_SCALE} for every s of pool_scales, got {pool_scales!r}")
        self.in_channels, self.pool_scales = in_channels, tuple(int(s) for s in pool_scales)
        self.psp_modules = nn.ModuleList(nn.Sequential(nn.AdaptiveAvgPool2d(s), ConvModule(in_channels, channels, 1))
                                         for s in self.pool_scales)
        self.bottleneck = ConvModule(in_channels + len(self.pool_scales) * channels, channels)
        self._init_tail(channels, num_classes, in_index, dropout_ratio, align_corners, loss_weight, ignore_index, impl, loss_decode)
        self.ppm = PyramidPooling(self, [seq[1] for seq in self.psp_modules], self.pool_scales, in_channels, channels, align_corners)

    def _cm(self):
        return self.bottleneck

    def _params(self):
        ps = []
        for seq in self.psp_modules:
            ps += [seq[1].conv.weight, seq[1].bn.weight, seq[1].bn.bias]
        return ps + [self.bottleneck.conv.weight, self.bottleneck.bn.weight, self.bottleneck.bn.bias, self.conv_seg.weight, self.conv_seg.bias]

    # ------------------------------------------------------------------ the torch arm: psp_head.py, line by line
    def _torch_forward(self, x):
        outs = [x]
        for s, seq in zip(self.pool_scales, self.psp_modules):
            conv, bn = seq[1].conv, seq[1].bn
            y = F.conv2d(F.adaptive_avg_pool2d(x, s), conv.weight)
            if bn.training:
                with torch.no_grad():
                    bn.num_batches_tracked += 1
            z = F.relu(F.batch_norm(y, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.training, bn.momentum, bn.eps))
            outs.append(F.interpolate(z, size=x.shape[2:], mode="bilinear", align_corners=self.align_corners))
        return self._torch_tail(torch.cat(outs, 1))

    # ------------------------------------------------------------------ the hip arm: the pyramid around the shared walk
    def _hip_forward(self, x, keep):
        B, Cin, h, w = x.shape
        self.ppm.check(B, h, w, self.training)
        ct = Cin + len(self.pool_scales) * self.channels
        xcat = self._buf("xcat", (B, h + 2, w + 2, ct), zero=True)
        pyramid = self.ppm.forward(x, xcat, keep)
        out, tail = self._tail_forward(xcat, B, ct, h, w, keep)
        return out, ((pyramid, tail) if keep else None)

    def _hip_backward(self, saved, dlogit, need_dx):
        pyramid, tail = saved
        branches = any(p.requires_grad for seq in self.psp_modules for p in seq[1].parameters())
        dxcat = self._tail_backward(tail, dlogit, need_dx or branches)
        if dxcat is None:
            return None
        return self.ppm.backward(pyramid, dxcat, need_dx)


class UPerHead(_BnClsHead):
    """mmseg 0.30 ``UPerHead`` (mmseg/models/decode_heads/uper_head.py) with its loss -- the reference's decode head
    (mem/semantic_segmentation/configs/_base_/models/upernet_beit.py:25-37: ``in_index=[0, 1, 2, 3], pool_scales=(1, 2, 3, 6),
    channels=512``).  With L = len(in_channels) levels, finest first, ``x_l = inputs[in_index[l]]``::

        lat_l   = ReLU(SyncBN(Conv2d(in_channels[l], channels, 1, bias=False)(x_l)))        l < L - 1     lateral_convs.{l}
        lat_L-1 = PSPHead's pyramid and bottleneck on x_L-1                                               psp_modules, bottleneck
        lat_l-1 = lat_l-1 + resize(lat_l, size of level l - 1)                              l = L - 1 .. 1
        out_l   = ReLU(SyncBN(Conv2d(channels, channels, 3, padding=1, bias=False)(lat_l))) l < L - 1     fpn_convs.{l}
        feat    = ReLU(SyncBN(Conv2d(L channels, channels, 3, padding=1, bias=False)(
                      cat([out_0] + [resize(out_l, size of level 0)] + [resize(lat_L-1, size of level 0)], 1))))   fpn_bottleneck
        logits  = conv_seg(Dropout2d(feat))

    under mmseg's state-dict keys and shapes: a reference checkpoint's ``decode_head.*`` loads with ``strict=True``.

    The interface, Dropout2d's keys and ``reduce`` are ``FCNHead``'s; ``forward`` takes the backbone's tuple and returns logits
    at level 0's size.  The hip arm (csrc/fpn.hip around the library's convolutions, ``PyramidPooling`` and the shared tail)
    takes CUDA fp32 maps whose sizes do not increase from level to level in either axis (equal sizes are fine), 2 <= L <= 4,
    every ``in_channels[l]`` and ``channels`` a multiple of 64, ``channels <= 512``, and ``PSPHead``'s pool scales.  Stored per
    level: the convolution outputs (bf16) and the top-down sums T_l (bf16, the FPN convolutions' operands); the activations
    ``lat_l``, ``out_l``, their upsampled maps and an fp32 concat never are.  ``reduce`` is called with "stats" five times in a
    training forward (laterals stacked [L-1, 3, C]; pyramid; bottleneck; fpn convs stacked; fpn_bottleneck) and with "bwd"
    four times in its backward (fpn_bottleneck; fpn convs stacked [L-1, 2, C]; laterals + bottleneck stacked [L, 2, C];
    pyramid)."""

    def __init__(self, in_channels=(768,) * 4, channels=512, num_classes=11, in_index=(0, 1, 2, 3), pool_scales=(1, 2, 3, 6),
                 dropout_ratio=0.1, align_corners=False, loss_weight=1.0, ignore_index=255, impl="hip", class_weight=None,
                 sampler=None, loss_decode=None, **kwargs):
        super().__init__()
        in_channels, in_index = tuple(in_channels), tuple(in_index)
        if len(in_channels) != len(in_index):
            raise ValueError(f"UPerHead: len(in_channels)={len(in_channels)} != len(in_index)={len(in_index)}")
        if not in_channels:
            raise ValueError("UPerHead: in_channels is empty")
        for c in in_channels:
            self._check_common(impl, dropout_ratio, c, channels, num_classes, class_weight, sampler, kwargs)
        pool_scales = tuple(pool_scales)
        if not pool_scales or any(int(s) != s or s < 1 for s in pool_scales):
            raise ValueError(f"pool_scales: positive integers, got {pool_scales!r}")
        if impl == "hip":
            if not 2 <= len(in_channels) <= ops.FPN_MAX_LEVELS:
                raise ValueError(f"UPerHead(impl='hip'): 2 <= levels <= {ops.FPN_MAX_LEVELS}, got in_channels={in_channels!r}")
            if len(pool_scales) > ops.PPM_MAX_SCALES:
                raise ValueError(f"UPerHead(impl='hip'): at most {ops.PPM_MAX_SCALES} pool_scales, got {pool_scales!r}")
            if any(not 1 <= s <= ops.PPM_MAX_SCALE for s in pool_scales):
                raise ValueError(f"UPerHead(impl='hip'): 1 <= s <= {ops.PPM_MAX_SCALE} for every s of pool_scales, got {pool_scales!r}")
        self.in_channels, self.pool_scales, self.levels = in_channels, tuple(int(s) for s in pool_scales), len(in_channels)
        self.psp_modules = nn.ModuleList(nn.Sequential(nn.AdaptiveAvgPool2d(s), ConvModule(in_channels[-1], channels, 1))
                                         for s in self.pool_scales)
        self.bottleneck = ConvModule(in_channels[-1] + len(self.pool_scales) * channels, channels)
        self.lateral_convs = nn.ModuleList(ConvModule(c, channels, 1) for c in in_channels[:-1])
        self.fpn_convs = nn.ModuleList(ConvModule(channels, channels) for _ in in_channels[:-1])
        self.fpn_bottleneck = ConvModule(len(in_channels) * channels, channels)
        self._init_tail(channels, num_classes, in_index, dropout_ratio, align_corners, loss_weight, ignore_index, impl, loss_decode)
        self.ppm = PyramidPooling(self, [seq[1] for seq in self.psp_modules], self.pool_scales, in_channels[-1], channels, align_corners)

    def _cm(self):
        return self.fpn_bottleneck

    def _upstream(self):
        """the ConvModules in front of ``fpn_bottleneck``'s operand"""
        return [seq[1] for seq in self.psp_modules] + [self.bottleneck] + list(self.lateral_convs) + list(self.fpn_convs)

    def _params(self):
        ps = []
        for m in self._upstream() + [self.fpn_bottleneck]:
            ps += [m.conv.weight, m.bn.weight, m.bn.bias]
        return ps + [self.conv_seg.weight, self.conv_seg.bias]

    # ------------------------------------------------------------------ the torch arm: uper_head.py, line by line
    def _torch_forward(self, xs):
        resize = lambda t, size: F.interpolate(t, size=size, mode="bilinear", align_corners=self.align_corners)
        laterals = [self._torch_cm(m, x) for m, x in zip(self.lateral_convs, xs)]
        x = xs[-1]
        psp = [x] + [resize(self._torch_cm(seq[1], F.adaptive_avg_pool2d(x, s)), x.shape[2:]) for s, seq in zip(self.pool_scales, self.psp_modules)]
        laterals.append(self._torch_cm(self.bottleneck, torch.cat(psp, 1)))
        for l in range(self.levels - 1, 0, -1):
            laterals[l - 1] = laterals[l - 1] + resize(laterals[l], laterals[l - 1].shape[2:])
        outs = [self._torch_cm(m, lat) for m, lat in zip(self.fpn_convs, laterals)] + [laterals[-1]]
        outs = [outs[0]] + [resize(o, outs[0].shape[2:]) for o in outs[1:]]
        return self._torch_tail(torch.cat(outs, 1))

    # ------------------------------------------------------------------ the hip arm
    def check(self, B, sizes, training):
        """refuse what the tables refuse, by name: level sizes that grow; and what the pyramid refuses on the last level"""
        for l in range(1, len(sizes)):
            if sizes[l][0] > sizes[l - 1][0] or sizes[l][1] > sizes[l - 1][1]:
                raise ValueError("UPerHead(impl='hip'): level %d of %dx%d is larger than level %d of %dx%d: the hip arm resizes upwards "
                                 "only, level sizes must not increase" % (l, sizes[l][0], sizes[l][1], l - 1, sizes[l - 1][0], sizes[l - 1][1]))
        self.ppm.check(B, sizes[-1][0], sizes[-1][1], training)

    def _stats_stacked(self, name, Y, B, sizes):
        C = self.channels
        ws = self._buf("stats.ws", (ops.BN_GROUPS * 2 * C,), torch.float32)
        out = self._buf(name, (len(Y), 3, C), torch.float32)
        for l, y in enumerate(Y):
            ops.bn_stats_nhwc(y, B, sizes[l][0], sizes[l][1], C, ws, None, True, out=out[l])
        return out

    def _level_vectors(self, name, mods, mean, rstd, mean_p, rstd_p):
        """(mean, rstd, gamma, beta) f32 [L, C] in the head's buffers ``name``: a row per level (``mods``: the lateral / FPN
        ConvModules, their vectors [L - 1, C]) and the pyramid bottleneck's as the last"""
        L, C, bp = self.levels, self.channels, self.bottleneck.bn
        out = [self._buf("%s.%s" % (name, k), (L, C), torch.float32) for k in ("mean", "rstd", "gamma", "beta")]
        out[0][:L - 1].copy_(mean)
        out[0][L - 1].copy_(mean_p)
        out[1][:L - 1].copy_(rstd)
        out[1][L - 1].copy_(rstd_p)
        for l, bn in enumerate([m.bn for m in mods] + [bp]):
            out[2][l].copy_(bn.weight.detach())
            out[3][l].copy_(bn.bias.detach())
        return tuple(out)

    def _totals(self, name, sums, inv_n):
        """``backward_totals`` for stacked sums [k, 2, C] with 1 / n [k, C], in the head's buffers: one ``reduce(., "bwd")``"""
        if inv_n is None:
            return None
        sent = self.reduce(self._buf(name + ".sent", tuple(sums.shape), torch.float32).copy_(sums), "bwd")
        return torch.mul(sent, inv_n[:, None, :], out=self._buf(name + ".tot", tuple(sums.shape), torch.float32))

    def _hip_forward(self, xs, keep):
        L, C, ac = self.levels, self.channels, self.align_corners
        B = xs[0].shape[0]
        sizes = [(int(x.shape[2]), int(x.shape[3])) for x in xs]
        self.check(B, sizes, self.training)
        Xp, Yl = [], []
        for l in range(L - 1):
            (h, w), Cin = sizes[l], self.in_channels[l]
            Xp.append(ops.map_to_nhwc_pad(xs[l], self._buf("lat.xp%d" % l, (B, h + 2, w + 2, Cin), zero=True)))
            Yl.append(self._buf("lat.y%d" % l, (B, h + 2, w + 2, C), zero=True))
            ops.conv2d_nhwc(Xp[l], self._packed(self.lateral_convs[l].conv, "conv1")[0], None, Yl[l], B, h, w, Cin, C, 1, 1, 0)
        with torch.no_grad():
            mean_l, rstd_l, inv_l = batch_vectors_stacked([m.bn for m in self.lateral_convs],
                                                          lambda: self._stats_stacked("lat.stats", Yl, B, sizes), self.reduce)
        (hL, wL), CinL = sizes[-1], self.in_channels[-1]
        ct = CinL + len(self.pool_scales) * C
        pxcat = self._buf("psp.xcat", (B, hL + 2, wL + 2, ct), zero=True)
        pyramid = self.ppm.forward(xs[-1], pxcat, keep)
        Yp = self._buf("psp.y", (B, hL + 2, wL + 2, C), zero=True)
        ops.conv2d_nhwc(pxcat, self._packed(self.bottleneck.conv, "conv3")[0], None, Yp, B, hL, wL, ct, C, 3, 1, 1)
        with torch.no_grad():
            mean_p, rstd_p, inv_p = batch_vectors(self.bottleneck.bn,
                                                  lambda: self._stats_stacked("psp.stats", [Yp], B, sizes[-1:])[0], self.reduce)
            lat_vecs = self._level_vectors("lat.vec", self.lateral_convs, mean_l, rstd_l, mean_p, rstd_p)
        # the top-down path: T_l = lat_l + resize(T_l+1); the coarsest lateral is read through its batch norm, never stored
        T = [None] * L
        for l in range(L - 2, -1, -1):
            T[l] = self._buf("fpn.t%d" % l, (B, sizes[l][0] + 2, sizes[l][1] + 2, C), zero=True)
            ops.fpn_topdown_fwd(l, sizes, Yl[l], lat_vecs, (Yp,) if l == L - 2 else T[l + 1], T[l], ac)
        Yf = []
        for l in range(L - 1):
            h, w = sizes[l]
            Yf.append(self._buf("fpn.y%d" % l, (B, h + 2, w + 2, C), zero=True))
            ops.conv2d_nhwc(T[l], self._packed(self.fpn_convs[l].conv, "conv3")[0], None, Yf[l], B, h, w, C, C, 3, 1, 1)
        with torch.no_grad():
            mean_f, rstd_f, inv_f = batch_vectors_stacked([m.bn for m in self.fpn_convs],
                                                          lambda: self._stats_stacked("fpn.stats", Yf, B, sizes), self.reduce)
            fpn_vecs = self._level_vectors("fpn.vec", self.fpn_convs, mean_f, rstd_f, mean_p, rstd_p)
        h0, w0 = sizes[0]
        xcat = self._buf("xcat", (B, h0 + 2, w0 + 2, L * C), zero=True)
        ops.fpn_concat_fwd(sizes, Yf + [Yp], fpn_vecs, xcat, ac)
        out, tail = self._tail_forward(xcat, B, L * C, h0, w0, keep)
        if not keep:
            return out, None
        return out, ((Xp, Yl, Yp, T, Yf, pxcat, pyramid, lat_vecs, fpn_vecs, inv_l, inv_p, inv_f, sizes, B), tail)

    def _wgrad(self, name, conv, dY, X, B, h, w, Cin, k):
        """the weight gradient of a k x k ConvModule's convolution from dY and its operand X, added to ``conv.weight.grad``"""
        if not conv.weight.requires_grad:
            return
        C = self.channels
        need = ops.conv_wgrad_workspace(B, h, w, Cin, C, k, 1, k // 2)
        wws = self._buf(name + ".ws", (need,), torch.uint8) if need else None
        gw = self._buf(name, (C, k * k * Cin), torch.float32)
        ops.conv_wgrad(dY, X, gw, B, h, w, Cin, C, k, 1, k // 2, small_padded=True, accumulate=False, workspace=wws)
        self._grad(conv.weight).add_(gw.view(C, k, k, Cin).permute(0, 3, 1, 2))

    def _hip_backward(self, saved, dlogit, needs):
        (Xp, Yl, Yp, T, Yf, pxcat, pyramid, lat_vecs, fpn_vecs, inv_l, inv_p, inv_f, sizes, B), tail = saved
        L, C, ac = self.levels, self.channels, self.align_corners
        upstream = any(p.requires_grad for m in self._upstream() for p in m.parameters())
        dxcat = self._tail_backward(tail, dlogit, any(needs) or upstream)
        grads = [None] * L
        if dxcat is None:
            return grads
        ws = self._buf("fpn.bwd.ws", (ops.BN_GROUPS * 2 * C,), torch.float32)
        # the FPN ConvModules: A_l = the transposed resize of dXcat's slice l
        sums_f = self._buf("fpn.sums", (L - 1, 2, C), torch.float32)
        A = []
        for l in range(L - 1):
            A.append(self._buf("fpn.a%d" % l, (B * sizes[l][0] * sizes[l][1], C), torch.float32))
            ops.fpn_resize_bwd(l, sizes, C, A[l], dxcat=dxcat, slice_=l, align_corners=ac)
            ops.fpn_bn_bwd_sums(l, sizes, Yf[l], fpn_vecs, A[l], sums_f[l], ws)
            add_affine_grads(self.fpn_convs[l].bn, sums_f[l])
        tot_f = self._totals("fpn.sums", sums_f, inv_f)
        dT_own = []
        for l in range(L - 1):
            h, w = sizes[l]
            dY = ops.fpn_bn_bwd_apply(l, sizes, Yf[l], fpn_vecs, A[l], None if tot_f is None else tot_f[l], 1.0,
                                      self._buf("fpn.dy%d" % l, (B, h + 2, w + 2, C), zero=True))
            self._wgrad("fpn.wgrad%d" % l, self.fpn_convs[l].conv, dY, T[l], B, h, w, C, 3)
            dT_own.append(self._buf("fpn.dt%d" % l, (B, h + 2, w + 2, C)))
            ops.conv2d_nhwc(dY, self._packed(self.fpn_convs[l].conv, "conv3")[1], None, dT_own[l], B, h, w, C, C, 3, 1, 1)
        # the top-down path backwards: dT_l = own + the transposed resize of dT_l-1; the coarsest level's own term is dXcat's
        dT = []
        for l in range(L):
            dT.append(self._buf("fpn.dlat%d" % l, (B * sizes[l][0] * sizes[l][1], C), torch.float32))
            fine = dT[l - 1] if l else None
            if l < L - 1:
                ops.fpn_resize_bwd(l, sizes, C, dT[l], own=dT_own[l], fine_rows=fine, align_corners=ac)
            else:
                ops.fpn_resize_bwd(l, sizes, C, dT[l], dxcat=dxcat, slice_=l, fine_rows=fine, align_corners=ac)
        # the laterals and the pyramid's bottleneck: one exchange
        sums_l = self._buf("lat.sums", (L, 2, C), torch.float32)
        Ys, mods = Yl + [Yp], list(self.lateral_convs) + [self.bottleneck]
        for l in range(L):
            ops.fpn_bn_bwd_sums(l, sizes, Ys[l], lat_vecs, dT[l], sums_l[l], ws)
            add_affine_grads(mods[l].bn, sums_l[l])
        inv = None
        if inv_l is not None:
            inv = self._buf("lat.inv_n", (L, C), torch.float32)
            inv[:L - 1].copy_(inv_l)
            inv[L - 1].copy_(inv_p)
        tot_l = self._totals("lat.sums", sums_l, inv)
        for l in range(L - 1):
            (h, w), Cin, conv = sizes[l], self.in_channels[l], self.lateral_convs[l].conv
            dY = ops.fpn_bn_bwd_apply(l, sizes, Yl[l], lat_vecs, dT[l], None if tot_l is None else tot_l[l], 1.0,
                                      self._buf("lat.dy%d" % l, (B, h + 2, w + 2, C), zero=True))
            self._wgrad("lat.wgrad%d" % l, conv, dY, Xp[l], B, h, w, Cin, 1)
            if needs[l]:
                dXp = self._buf("lat.dxp%d" % l, (B, h + 2, w + 2, Cin))
                ops.conv2d_nhwc(dY, self._packed(conv, "conv1")[1], None, dXp, B, h, w, C, Cin, 1, 1, 0)
                grads[l] = ops.nhwc_pad_to_map(dXp, out=self._buf("lat.dmap%d" % l, (B, Cin, h, w), torch.float32)).detach()
        (hL, wL), ct = sizes[-1], pxcat.shape[3]
        dY = ops.fpn_bn_bwd_apply(L - 1, sizes, Yp, lat_vecs, dT[L - 1], None if tot_l is None else tot_l[L - 1], 1.0,
                                  self._buf("psp.dy", (B, hL + 2, wL + 2, C), zero=True))
        self._wgrad("psp.wgrad", self.bottleneck.conv, dY, pxcat, B, hL, wL, ct, 3)
        branches = any(p.requires_grad for seq in self.psp_modules for p in seq[1].parameters())
        if needs[L - 1] or branches:
            dpx = self._buf("psp.dxcat", (B, hL + 2, wL + 2, ct))
            ops.conv2d_nhwc(dY, self._packed(self.bottleneck.conv, "conv3")[1], None, dpx, B, hL, wL, C, ct, 3, 1, 1)
            grads[L - 1] = self.ppm.backward(pyramid, dpx, needs[L - 1])
        return grads

    # ------------------------------------------------------------------ mmseg's interface: the backbone's tuple
    def forward(self, inputs):
        xs = [inputs[i] for i in self.in_index]
        if self.impl == "torch":
            return self._torch_forward(xs)
        for l, x in enumerate(xs):
            if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == self.in_channels[l]
                    and x.shape[0] == xs[0].shape[0]):
                from ._lib import MemhipError
                raise MemhipError("UPerHead(impl='hip') takes the engine's CUDA fp32 maps [B, %d, h, w] at level %d (no CPU fallback)"
                                  % (self.in_channels[l], l))
        xs = [x.contiguous() for x in xs]
        params = self._params()
        if torch.is_grad_enabled() and (any(x.requires_grad for x in xs) or any(p.requires_grad for p in params)):
            return _LevelsFunction.apply(self, len(xs), *xs, *params)
        return self._hip_forward([x.detach() for x in xs], keep=False)[0]


class SegModel(nn.Module):
    """mmseg's ``EncoderDecoder``, thin: ``backbone`` (an ``EvBEiT``: images -> a tuple of maps), ``decode_head`` and an optional
    ``auxiliary_head`` (each a ``UPerHead``, ``PSPHead`` or ``FCNHead``; the reference's model is ``SegModel(EvBEiT, UPerHead,
    FCNHead)``).  ``forward_train(img, seg_label)`` -> ``{"decode.loss_seg", "decode.acc_seg", "aux.loss_seg", "aux.acc_seg"}``;
    ``encode_decode(img)`` -> the decode head's logits at the head's resolution (``test_cfg.mode='whole'``: the resize to the
    label's size is ``SegEvaluator``'s).  One object for an optimizer and an evaluator."""

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
