"""Mixup / CutMix for the finetuning loop -- timm.data.Mixup as mem/run_class_finetuning.py:504-511 of the reference builds it
(mixup 0.8, cutmix 1.0, label smoothing folded into the targets), restated from timm's published definition (timm is not
vendored).  Same constructor keywords and call signature; ``train_one_epoch(mixup_fn=Mixup(...))``.

The host only DRAWS the parameters (``draw``); the arithmetic is two HIP kernels (include/memhip.h): ``memhip_mixup`` mixes
the fp32 image batch in place with its flipped self (no ``x.flip(0)`` / ``x.clone()`` copy: one pass, 2 x batch bytes), and
``memhip_mix_targets`` builds the soft targets.  Parameters go up through a pinned staging ring and are never read back.

Random draws come from ``numpy.random`` -- the GLOBAL state by default, like timm, so an entrypoint that seeds numpy
reproduces timm's parameter sequence; ``rng=`` takes a ``numpy.random.RandomState`` instead.  Draw order (fixed; pinned by
tests/test_recipe_cpu.py against a restatement):

* ``mode='batch'`` -- one (lam, box) for the batch:
  1. ``rand() < prob``, else lam = 1 and no box (nothing further is drawn);
  2. both alphas > 0: ``use_cutmix = rand() < switch_prob``, then ``beta(a, a)`` with the chosen alpha; only one alpha > 0:
     that one, no switch draw;
  3. if lam == 1 the batch is left alone; with cutmix the box is drawn (below).
* ``mode='elem'`` -- vectorised over the B samples: ``rand(B) < switch_prob`` (only when both alphas > 0), then
  ``beta(cutmix_alpha, size=B)`` AND ``beta(mixup_alpha, size=B)`` (both alphas > 0: timm selects with ``np.where``, which
  evaluates both draws, cutmix first) or the single ``beta(alpha, size=B)``; then ``where(rand(B) < prob, lam_mix, 1)`` in
  float32.  Boxes are then drawn sample by sample, in order, for the samples with cutmix and lam != 1.
* ``mode='pair'`` -- the same for B/2 samples; sample B-1-i gets the lam and the box of sample i.
* cutmix box for lam: ``ratio = sqrt(1 - lam)``; ``cut_h, cut_w = int(H * ratio), int(W * ratio)``; ``cy = randint(0, H)``,
  then ``cx = randint(0, W)``; ``yl, yh = clip(cy - cut_h // 2, 0, H), clip(cy + cut_h // 2, 0, H)``, likewise x.
* cutmix box with ``cutmix_minmax``: ``cut_h = randint(int(H * min), int(H * max))``, ``cut_w`` likewise,
  ``yl = randint(0, H - cut_h)``, ``xl`` likewise.
* ``correct_lam`` (and always with ``cutmix_minmax``): ``lam = 1 - (yh - yl)(xh - xl) / (H * W)``.

Two points where timm's published code differs from a shorter reading of the recipe, and timm is followed: with
``cutmix_minmax`` timm sets ``cutmix_alpha = 1.0`` -- cutmix is then on, but a ``mixup_alpha`` > 0 still takes part in the
switch draw; and in ``elem`` / ``pair`` with both alphas BOTH beta vectors are drawn.  In ``elem`` / ``pair`` lam is a
float32 value while the box is computed from it (timm keeps ``lam_batch`` as a float32 array), in ``batch`` a Python float.

Not carried: uint8 image batches (timm's FastCollateMixup).
"""
import numpy as np
import torch

from . import ops
from .utils import HostStager


class Mixup:
    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch',
                 correct_lam=True, label_smoothing=0.1, num_classes=1000, rng=None):
        self.mixup_alpha = mixup_alpha
        self.cutmix_alpha = cutmix_alpha
        self.cutmix_minmax = cutmix_minmax
        if self.cutmix_minmax is not None:
            assert len(self.cutmix_minmax) == 2
            self.cutmix_alpha = 1.0                      # timm: force cutmix alpha == 1.0 when minmax is active
        assert mode in ('batch', 'pair', 'elem'), mode
        self.mix_prob = prob
        self.switch_prob = switch_prob
        self.label_smoothing = label_smoothing
        self.num_classes = num_classes
        self.mode = mode
        self.correct_lam = correct_lam
        self.mixup_enabled = True                        # timm: set False to disable mixing
        self.rng = rng if rng is not None else np.random
        self._stager = None

    # ------------------------------------------------------------------ host: parameter draws
    def _lam_mix(self, size=None):
        """(use_cutmix, lam_mix) by timm's three-way choice; size None: scalars."""
        r = self.rng
        if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
            use_cutmix = (r.rand() if size is None else r.rand(size)) < self.switch_prob
            if size is None:
                a = self.cutmix_alpha if use_cutmix else self.mixup_alpha
                return use_cutmix, r.beta(a, a)
            return use_cutmix, np.where(use_cutmix, r.beta(self.cutmix_alpha, self.cutmix_alpha, size=size),
                                        r.beta(self.mixup_alpha, self.mixup_alpha, size=size))
        if self.mixup_alpha > 0.:
            use_cutmix = False if size is None else np.zeros(size, dtype=bool)
            return use_cutmix, r.beta(self.mixup_alpha, self.mixup_alpha, size=size)
        assert self.cutmix_alpha > 0., "One of mixup_alpha > 0., cutmix_alpha > 0., cutmix_minmax not None should be true."
        use_cutmix = True if size is None else np.ones(size, dtype=bool)
        return use_cutmix, r.beta(self.cutmix_alpha, self.cutmix_alpha, size=size)

    def _box_and_lam(self, H, W, lam):
        """timm cutmix_bbox_and_lam: ((yl, yh, xl, xh), lam)."""
        r = self.rng
        if self.cutmix_minmax is not None:
            lo, hi = self.cutmix_minmax
            cut_h = r.randint(int(H * lo), int(H * hi))
            cut_w = r.randint(int(W * lo), int(W * hi))
            yl = r.randint(0, H - cut_h)
            xl = r.randint(0, W - cut_w)
            yh, xh = yl + cut_h, xl + cut_w
        else:
            ratio = np.sqrt(1 - lam)
            cut_h, cut_w = int(H * ratio), int(W * ratio)
            cy = r.randint(0, H)
            cx = r.randint(0, W)
            yl, yh = np.clip(cy - cut_h // 2, 0, H), np.clip(cy + cut_h // 2, 0, H)
            xl, xh = np.clip(cx - cut_w // 2, 0, W), np.clip(cx + cut_w // 2, 0, W)
        if self.correct_lam or self.cutmix_minmax is not None:
            lam = 1. - (yh - yl) * (xh - xl) / float(H * W)
        return (yl, yh, xl, xh), lam

    def _draw(self, B, H, W):
        """(lam f32 [B], box i32 [B, 4], cut bool [B]): cut marks the samples mixed by copying a box (its area may be zero)."""
        lam = np.ones(B, dtype=np.float32)
        box = np.zeros((B, 4), dtype=np.int32)
        cut = np.zeros(B, dtype=bool)
        if not self.mixup_enabled:
            return lam, box, cut
        if self.mode == 'batch':
            if self.rng.rand() < self.mix_prob:
                use_cutmix, lam_mix = self._lam_mix()
                l = float(lam_mix)
                if l != 1.:
                    if use_cutmix:
                        box[:], l = self._box_and_lam(H, W, l)
                        cut[:] = True
                    lam[:] = l
            return lam, box, cut
        n = B if self.mode == 'elem' else B // 2
        use_cutmix, lam_mix = self._lam_mix(n)
        lam_n = np.where(self.rng.rand(n) < self.mix_prob, lam_mix.astype(np.float32), np.ones(n, dtype=np.float32))
        for i in range(n):
            if lam_n[i] != 1. and use_cutmix[i]:
                box[i], lam_n[i] = self._box_and_lam(H, W, lam_n[i])
                cut[i] = True
        lam[:n] = lam_n
        if self.mode == 'pair':
            lam[n:], box[n:], cut[n:] = lam_n[::-1], box[:n][::-1], cut[:n][::-1]
        return lam, box, cut

    def draw(self, B, H, W):
        """Host only: this call's (lam float32 [B], box int32 [B, 4] = (yl, yh, xl, xh)); an all-zero box: blend with lam."""
        lam, box, _ = self._draw(B, H, W)
        return lam, box

    # ------------------------------------------------------------------ device
    def __call__(self, x, target):
        assert len(x) % 2 == 0, 'Batch size should be even when using this'
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4, "Mixup: fp32 [B, C, H, W] image batch on the GPU"
        if not x.is_contiguous():
            x = x.contiguous()
        B, _, H, W = x.shape
        lam, box, cut = self._draw(B, H, W)
        # a cutmix sample whose box has no area (a cut of zero pixels, or one clipped away at the border) copies nothing in
        # timm: the image kernel sees lam = 1 ("leave alone") for it, the targets keep the drawn lam
        empty = (box[:, 1] <= box[:, 0]) | (box[:, 3] <= box[:, 2])
        lam_img = np.where(cut & empty, np.float32(1), lam).astype(np.float32)
        words = np.concatenate([lam.view(np.int32), lam_img.view(np.int32), box.reshape(-1)])
        if self._stager is None or self._stager.host[0].numel() < words.nbytes:
            self._stager = HostStager(words.nbytes, x.device)
        dev = self._stager.put(words)
        lam_t, lam_i, box_d = dev[:B].view(torch.float32), dev[B:2 * B].view(torch.float32), dev[2 * B:]
        ops.mixup(x, lam_i, box_d, lam_img, box)
        soft = torch.empty(B, self.num_classes, dtype=torch.float32, device=x.device)
        ops.mix_targets(target.to(device=x.device, dtype=torch.int64).contiguous(), lam_t, self.num_classes,
                        self.label_smoothing, soft)
        return x, soft
