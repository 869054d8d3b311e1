"""Event dVAE tokenizer, inference side -- adjacent dependency of the pretraining loop (reference:
eventvae/vae/vae_model.py:29-113,153-189; called every step at mem/engine_for_pretraining.py:144).

`DiscreteVAE` is the torch module with the reference's module tree, so reference checkpoints ('hparams' / 'weights') load by
key; `HipTokenizer` runs it on the hand-written HIP path (csrc/conv*.hip, csrc/convt.hip): the encoder
(`get_codebook_indices`: fp32, certified fp16x2 or bf16 implicit-GEMM convolutions + argmax) and the decoder (`decode`,
`reconstruct`: bf16, the transposed convolutions as four 2x2 phase GEMMs).  mem_amd/eval_tokenizer.py evaluates a checkpoint
with them (reconstruction loss, KL to uniform, codebook usage; vae_model.py:216-266).
Training the dVAE (gumbel-softmax forward, the backward, Adam) runs on `vae_train.DVAEEngine` / `python -m mem_amd.train_vae`,
with an explicit backward on the HIP kernels; the torch module itself has no training forward.  This file holds the host side
of that backward's weights: `dgrad_weight` / `pack_dgrad_weight` re-read a layer's weight so that its data gradient is one of
the forward kernels."""
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F
from torch import nn


def pack_convt_weight(w, cin_pad=None, cout_pad=None):
    """The weight layout of ops.convt2d_nhwc (csrc/convt.hip).  w: torch's ConvTranspose2d(Cin, Cout, 4, stride=2, padding=1)
    weight [Cin, Cout, 4, 4] -> [4, Cout, 4 * Cin] in w's dtype, K-contiguous:

        packed[2 * py + px, co, (2 * dy + dx) * Cin + ci] = w[ci, co, 3 - py - 2 * dy, 3 - px - 2 * dx]

    Output phase (py, px) = the parity of the output pixel (2y + py, 2x + px); (dy, dx) in {0, 1}^2 walks the 2 x 2 input
    window whose top-left pixel is PADDED position (y + py, x + px) of the one-pixel-border input, so that

        out[b, 2y+py, 2x+px, co] = bias[co] + sum_{dy, dx, ci} in_pad[b, y+py+dy, x+px+dx, ci] * packed[2py+px, co, (2dy+dx) Cin + ci]

    cin_pad / cout_pad: zero-pad the channel counts first (the kernel wants Cin % 64 == 0 and Cout % 8 == 0)."""
    ci, co, kh, kw = w.shape
    assert kh == 4 and kw == 4, "ConvTranspose2d(4, stride 2, padding 1) only"
    cip, cop = cin_pad or ci, cout_pad or co
    if (cip, cop) != (ci, co):
        w = F.pad(w, (0, 0, 0, 0, 0, cop - co, 0, cip - ci))
    phases = []
    for py in (0, 1):
        for px in (0, 1):
            taps = [w[:, :, 3 - py - 2 * dy, 3 - px - 2 * dx] for dy in (0, 1) for dx in (0, 1)]     # each [Cin, Cout]
            phases.append(torch.stack(taps).permute(2, 0, 1).reshape(cop, 4 * cip))                # [Cout, (dy, dx, ci)]
    return torch.stack(phases).contiguous()


def pack_conv_weight(w):
    """The weight layout of ops.conv2d_nhwc (and of ops.conv_wgrad's gradient): torch's Conv2d weight [Cout, Cin, k, k] ->
    [Cout, k*k*Cin], (ky, kx, c)-major."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def dgrad_weight(kind, w):
    """Data gradients of the dVAE's layers are forward kernels with a re-read weight.  Returns (op, weight in torch layout) with
    which dX = op(g, weight), for the layer kinds of the model:

        "conv4s2"  Conv2d(4, stride 2, pad 1), w [Co, Ci, 4, 4]:  dX = conv_transpose2d(g, w, stride 2, pad 1) -- w already has
                   ConvTranspose2d's [in = Co, out = Ci, 4, 4] layout
        "convt"    ConvTranspose2d(4, 2, 1), w [Ci, Co, 4, 4]:    dX = conv2d(g, w, stride 2, pad 1) -- w read as [out = Ci, in = Co]
        "conv3"    Conv2d(3, 1, 1), w [Co, Ci, 3, 3]:             dX = conv2d(g, w', pad 1), w'[ci, co, ky, kx] = w[co, ci, 2-ky, 2-kx]
        "conv1"    Conv2d(1), w [Co, Ci, 1, 1]:                   dX = conv2d(g, w^T)

    Plain torch on the weights, once per step; not on the hot path."""
    if kind == "conv4s2":
        return "conv_transpose2d", w
    if kind == "convt":
        return "conv2d", w
    if kind == "conv3":
        return "conv2d", w.flip(2, 3).transpose(0, 1).contiguous()
    if kind == "conv1":
        return "conv2d", w.transpose(0, 1).contiguous()
    raise KeyError(kind)


def pack_dgrad_weight(kind, w, cin_pad=None, cout_pad=None):
    """dgrad_weight in the layout of the kernel that runs it: ops.convt2d_nhwc's phase-packed [4, Ci, 4*Co] for "conv4s2",
    ops.conv2d_nhwc's [out, k*k*in] for the others.  cin_pad / cout_pad zero-pad the channels of g / of dX."""
    op, wd = dgrad_weight(kind, w)
    if op == "conv_transpose2d":
        return pack_convt_weight(wd, cin_pad=cin_pad, cout_pad=cout_pad)
    co, ci = wd.shape[:2]
    if (cin_pad or ci, cout_pad or co) != (ci, co):
        wd = F.pad(wd, (0, 0, 0, 0, 0, (cin_pad or ci) - ci, 0, (cout_pad or co) - co))
    return pack_conv_weight(wd)


class ResBlock(nn.Module):
    def __init__(self, chan):
        super().__init__()
        self.net = nn.Sequential(nn.Conv2d(chan, chan, 3, padding=1), nn.ReLU(), nn.Conv2d(chan, chan, 3, padding=1),
                                 nn.ReLU(), nn.Conv2d(chan, chan, 1))

    def forward(self, x):
        return self.net(x) + x


class DiscreteVAE(nn.Module):
    def __init__(self, input_H=256, input_W=256, num_tokens=512, codebook_dim=512, num_layers=3,
                 num_resnet_blocks=0, hidden_dim=64, channels=3, loss="mse", temperature=0.9,
                 straight_through=False, kl_div_loss_weight=0.0, normalization=None):
        super().__init__()
        assert input_H % (2 ** num_layers) == 0 and input_W % (2 ** num_layers) == 0 and num_layers >= 1
        self.input_H, self.input_W, self.input_size = input_H, input_W, (input_H, input_W)
        self.num_tokens, self.num_layers = num_tokens, num_layers
        self.normalization = normalization
        self.loss, self.temperature, self.straight_through = loss, temperature, straight_through
        self.kl_div_loss_weight = kl_div_loss_weight
        # vae_model.py:107-108
        self.loss_fn = {"mse": F.mse_loss, "smooth_l1": F.smooth_l1_loss, "cosine": self.cosine_reconstruction_loss}[loss]
        self.codebook = nn.Embedding(num_tokens, codebook_dim)
        has_res = num_resnet_blocks > 0
        enc_chans = [channels] + [hidden_dim] * num_layers
        dec_chans = [codebook_dim if not has_res else hidden_dim] + [hidden_dim] * num_layers
        enc, dec = [], []
        for (ei, eo), (di, do) in zip(zip(enc_chans[:-1], enc_chans[1:]), zip(dec_chans[:-1], dec_chans[1:])):
            enc.append(nn.Sequential(nn.Conv2d(ei, eo, 4, stride=2, padding=1), nn.ReLU()))
            dec.append(nn.Sequential(nn.ConvTranspose2d(di, do, 4, stride=2, padding=1), nn.ReLU()))
        for _ in range(num_resnet_blocks):
            dec.insert(0, ResBlock(dec_chans[1]))
            enc.append(ResBlock(enc_chans[-1]))
        if has_res:
            dec.insert(0, nn.Conv2d(codebook_dim, dec_chans[1], 1))
        enc.append(nn.Conv2d(enc_chans[-1], num_tokens, 1))
        dec.append(nn.Conv2d(dec_chans[-1], channels, 1))
        self.encoder, self.decoder = nn.Sequential(*enc), nn.Sequential(*dec)

    @staticmethod
    def cosine_reconstruction_loss(target, rec):
        """vae_model.py:116-119"""
        target = target / (target.norm(dim=-1, keepdim=True) + 1e-9)
        rec = rec / (rec.norm(dim=-1, keepdim=True) + 1e-9)
        return (1 - (target * rec).sum(-1)).mean()

    def norm(self, images):
        if self.normalization is None:
            return images
        means, stds = (torch.as_tensor(t).to(images).view(1, -1, 1, 1) for t in self.normalization)
        return (images - means) / stds

    @torch.no_grad()
    def get_codebook_indices(self, images):
        """vae_model.py:153-158: argmax over the token logits, eval mode, no grad -> i64 [B, h*w]."""
        was = self.training
        self.eval()
        logits = self.encoder(self.norm(images))
        self.train(was)
        return logits.argmax(dim=1).flatten(1)

    def forward(self, img, return_logits=False, **kw):
        assert img.shape[-1] == self.input_W and img.shape[-2] == self.input_H
        if not return_logits:
            raise NotImplementedError("the torch module has no training forward: dVAE training (gumbel-softmax forward, losses, "
                                      "explicit backward) is mem_amd.vae_train.DVAEEngine / python -m mem_amd.train_vae; "
                                      "reconstruction: HipTokenizer.reconstruct / mem_amd.eval_tokenizer")
        return self.encoder(self.norm(img))

    def decode(self, img_seq):
        emb = self.codebook(img_seq)
        b, n, d = emb.shape
        h, w = self.input_H // 2 ** self.num_layers, self.input_W // 2 ** self.num_layers
        return self.decoder(emb.transpose(1, 2).reshape(b, d, h, w))


class ConvLayer(NamedTuple):
    """One packed convolution of the encoder: weight [Cout, k*k*cin] ((ky, kx, c)-major; fp16x2: two planes), fp32 bias."""
    w: torch.Tensor
    b: Optional[torch.Tensor]
    cin: int
    cout: int
    k: int
    stride: int
    pad: int

    def out_hw(self, h, w):
        """Output size of this convolution on an h x w input -- the one place that computes it."""
        return (h + 2 * self.pad - self.k) // self.stride + 1, (w + 2 * self.pad - self.k) // self.stride + 1


class HipTokenizer:
    """`DiscreteVAE.get_codebook_indices` on the hand-written HIP path: NHWC activations with a one-pixel zero
    border, implicit-GEMM convolutions on MFMA tiles with fused bias / ReLU / residual, argmax over the token logits.
    Built from a (frozen) `DiscreteVAE` whose weights it packs once.

    precision="fp32" (default, csrc/conv_f32.hip): fp32 operands and accumulation (v_mfma_f32_16x16x4_f32), i.e. the
      reference's arithmetic -- it runs the tokenizer in fp32, outside the autocast block
      (mem/engine_for_pretraining.py:140-147).  The ids are integers: the parity bar is EQUALITY with the fp32
      reference (tests/test_tokenizer_gpu.py).
    precision="fp16x2" (csrc/conv_f16x2.hip): every value as two fp16 planes (hi, (v - hi) * 2048), three fp16 MFMAs per
      product: logits within ~3e-5 of fp32 at a logit rms of ~1.8 (fp32 summation-order noise is ~3e-6); ~2x faster than
      fp32.  CERTIFIED (`certify=True`, the default of this mode): a label is accepted only where its top-2 gap exceeds
      kappa x the row's rms; every sample holding a token below that margin is recomputed ON THE DEVICE, without a host
      synchronisation, by the fp32 kernels (an inner fp32 tokenizer with a capacity of `exact_capacity` samples per round
      -- default 256 = one round per batch: every extra round is 17 launches of empty grids, ~0.2 ms; its fp32 buffers are
      27 MB per sample of capacity at 224^2, i.e. 6.9 GB at the default capacity -- dynamic batch read from device memory)
      and its labels are replaced.  A label can only differ from the fp32 mode's where the gap is below twice the logit
      deviation E of the split-precision path, so with kappa >= 2 E / rms the ids equal the fp32 mode's.  E is NOT a
      closed-form constant: a worst-case bound through 13 convolutions (operand planes carry 2^-22 relative error, the
      dropped lo x lo term another 2^-22, two fp32 summation orders) compounds L1 weight norms and is vacuous, so kappa is
      MEASURED PER MODEL (round 6): at construction both paths run on a calibration batch (uniform and sparse synthetic
      images, or `calibration_images`), kappa = max(KAPPA_FLOOR, 4 x the worst |logit_fp16x2 - logit_fp32| / rms) -- a 2 x
      margin on the 2 E condition, adapted to the weights' dynamic range -- and the claim is AUDITED at run time: every
      `audit_every`-th call one sample is recomputed in fp32 on the device and label mismatches are counted
      (`certification_stats()["audit_mismatches"]`, expected 0).  `certify=False` is the raw mode.
    precision="bf16" (csrc/conv.hip): bf16 operands, fp32 accumulation; ~6x faster, 97-99 % of the ids agree (the rest
      are near ties) -- an explicit opt-in (`--tokenizer_impl hip_bf16`), never the default.

    `decode(ids)` / `reconstruct(images)` are `DiscreteVAE.decode` on the same path, in bf16 whatever the encoder's precision
    (the reference evaluates the decoder under autocast): codebook rows gathered into the padded NHWC format, the 1x1
    convolution and ResBlocks through the bf16 convolutions, the ConvTranspose2d(4, s2, p1) layers through csrc/convt.hip.
    The decoder's weights and buffers are packed / allocated on the first `decode`, for chunks of `decode_batch` samples."""

    # flag a token when gap <= kappa * rms(row).  kappa is calibrated per model (see the class docstring); CERT_KAPPA is the value
    # round 5 used for every model (4 x the worst deviation seen then, 1.75e-5 of the rms on the ViT-B fixture) and stays as the
    # reference point of the tests; KAPPA_FLOOR keeps a lucky calibration batch from shrinking the margin below ~40 operand ulps
    CERT_KAPPA = 7e-5
    KAPPA_FLOOR = 1e-5

    def __init__(self, vae: "DiscreteVAE", max_batch=256, precision="fp32", certify=True, exact_capacity=256, kappa=None,
                 calibration_images=None, audit_every=64, decode_batch=16):
        from . import ops
        self.ops = ops
        self._model = vae                                  # decode() packs the decoder from it on first use
        self.decode_batch = int(decode_batch)
        self._dec = None
        assert precision in ("fp32", "bf16", "fp16x2")
        self.precision = precision
        self.certify = bool(certify) and precision == "fp16x2"
        self.exact_capacity = int(exact_capacity)
        self._vae = vae if self.certify else None
        self._exact = None
        self.dt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16x2": torch.float16}[precision]
        self.planes = 2 if precision == "fp16x2" else 1
        dev = next(vae.parameters()).device
        assert dev.type == "cuda", "HipTokenizer needs the model on the GPU"
        self.dev, self.H, self.W = dev, vae.input_H, vae.input_W
        self.num_tokens = vae.num_tokens
        self.norm = None
        if vae.normalization is not None:
            m, s = (torch.as_tensor(t, dtype=torch.float32, device=dev).contiguous() for t in vae.normalization)
            self.norm = (m, s)
        # the encoder in order: ("conv", ConvLayer) = strided conv + ReLU, ("res", (ConvLayer,) * 3) = ResBlock, ("head", ConvLayer)
        self.layers = []
        self.cin0 = None
        for m in vae.encoder:
            if isinstance(m, nn.Sequential):               # Conv2d(4, s2, p1) + ReLU
                self.layers.append(("conv", self._pack(m[0])))
                if self.cin0 is None:
                    self.cin0 = m[0].in_channels
            elif isinstance(m, ResBlock):
                self.layers.append(("res", tuple(self._pack(m.net[i]) for i in (0, 2, 4))))
            else:                                          # final Conv2d(hidden, num_tokens, 1)
                self.layers.append(("head", self._pack(m)))
        assert self.cin0 is not None and self.cin0 <= 4, "first layer must have <= 4 input channels"
        self.max_batch = 0
        self.kappa = float(kappa) if kappa is not None else self.CERT_KAPPA
        self.audit_every = int(audit_every)
        self._alloc(max_batch)
        if self.certify and kappa is None:
            self.kappa, self.calibration = self._calibrate(calibration_images)

    @torch.no_grad()
    def _calibrate(self, images=None):
        """kappa of THIS model: both paths on a calibration batch, 4 x the worst logit deviation relative to the row rms."""
        ex = self._exact
        n = max(1, min(8, ex.max_batch, self.max_batch))
        if images is None:
            g = torch.Generator(device=self.dev).manual_seed(20261)
            c = self.cin0
            u = torch.rand((n, c, self.H, self.W), generator=g, device=self.dev)
            sparse = u * (torch.rand((n, c, self.H, self.W), generator=g, device=self.dev) < 0.3)     # event-frame-like
            images = torch.cat([u[: (n + 1) // 2], sparse[: n // 2]]) if n > 1 else u
        images = images[:n].to(self.dev, torch.float32).contiguous()
        n = images.shape[0]
        M = n * self.hw_out[0] * self.hw_out[1]
        certify, self.certify = self.certify, False
        try:
            self.get_codebook_indices(images)
        finally:
            self.certify = certify
        ex.get_codebook_indices(images)
        l32 = ex.logits[:M]
        rms = l32.pow(2).mean(1, keepdim=True).sqrt().clamp_min(1e-30)
        dev = float(((self.logits[:M] - l32).abs() / rms).max())
        return max(self.KAPPA_FLOOR, 4.0 * dev), {"samples": n, "max_deviation_over_rms": dev}

    def _pack(self, conv):
        w = conv.weight.detach()                           # [Cout, Cin, k, k]
        co, ci, k, _ = w.shape
        w = w.permute(0, 2, 3, 1)                          # (ky, kx, c)-major
        if ci < 4:
            w = torch.nn.functional.pad(w, (0, 4 - ci))
            ci = 4
        wp = w.reshape(co, k * k * ci)
        if self.precision == "fp16x2":
            hi = wp.half()
            wp = torch.stack([hi, ((wp.float() - hi.float()) * 2048.0).half()]).contiguous()       # [2, Cout, K]
        else:
            wp = wp.to(self.dt).contiguous()
        b = conv.bias.detach().float().contiguous() if conv.bias is not None else None
        return ConvLayer(wp, b, ci, co, k, conv.stride[0], conv.padding[0])

    def _alloc(self, B):
        """Zero-bordered activation buffers for batch B (allocated once; only interiors are written)."""
        if B <= self.max_batch:
            return
        dev, bf = self.dev, self.dt
        self.max_batch = B
        H, W = self.H, self.W
        pl = (2,) if self.planes == 2 else ()             # fp16x2: [2 (hi / lo plane), B, H+2, W+2, C]
        self.x0 = torch.zeros(pl + (B, H + 2, W + 2, 4), dtype=bf, device=dev)
        self.bufs = {}
        h, w = H, W
        for kind, L in self.layers:                       # one buffer per strided level; the ResBlocks' level gets 3
            if kind == "head":
                continue
            if kind == "conv":
                h, w = L.out_hw(h, w)
            cout = L.cout if kind == "conv" else L[0].cout
            pool = self.bufs.setdefault((h, w, cout), [])
            while len(pool) < (1 if kind == "conv" else 3):
                pool.append(torch.zeros(pl + (B, h + 2, w + 2, cout), dtype=bf, device=dev))
        self.hw_out = (h, w)
        lt = torch.float32 if self.precision in ("fp32", "fp16x2") else bf
        self.logits = torch.empty((B * h * w, self.num_tokens), dtype=lt, device=dev)
        self.ids = torch.empty((B * h * w,), dtype=torch.int64, device=dev)
        self.gap = torch.empty((B * h * w,), dtype=torch.float32, device=dev) if lt == torch.float32 else None
        if self.certify:
            self.rms = torch.empty((B * h * w,), dtype=torch.float32, device=dev)
            self.flag_list = torch.zeros((B,), dtype=torch.int32, device=dev)
            self.flag_count = torch.zeros((1,), dtype=torch.int32, device=dev)
            self.n_round = torch.zeros((1,), dtype=torch.int32, device=dev)
            if not hasattr(self, "cert_stats"):
                # [flagged samples, calls, audit label mismatches, audited samples] so far
                self.cert_stats = torch.zeros((4,), dtype=torch.int64, device=dev)
                self._calls = 0
            R = max(1, min(self.exact_capacity, B))
            if self._exact is None or self._exact.max_batch < R:
                self._exact = HipTokenizer(self._vae, max_batch=R, precision="fp32")

    def _walk(self, n, **kw):
        """The encoder from self.x0 to self.logits on `n` samples (the batch, or the capacity of a dynamic-batch call); kw goes
        to every convolution (n_active).  Owns the ResBlock buffer rotation: t1, t2 = the first pool buffers that are not
        the block's input.  Returns the output size (h, w)."""
        conv = self.ops.conv2d_nhwc
        cur, h, w = self.x0, self.H, self.W
        for kind, L in self.layers:
            if kind == "conv":
                ho, wo = L.out_hw(h, w)
                out = self.bufs[(ho, wo, L.cout)][0]
                conv(cur, L.w, L.b, out, n, h, w, L.cin, L.cout, L.k, L.stride, L.pad, relu=True, **kw)
                cur, h, w = out, ho, wo
            elif kind == "res":
                c1, c2, c3 = L
                pool = self.bufs[(h, w, c1.cout)]
                t1 = next(t for t in pool if t is not cur)
                t2 = next(t for t in pool if t is not cur and t is not t1)
                conv(cur, c1.w, c1.b, t1, n, h, w, c1.cin, c1.cout, c1.k, c1.stride, c1.pad, relu=True, **kw)
                conv(t1, c2.w, c2.b, t2, n, h, w, c2.cin, c2.cout, c2.k, c2.stride, c2.pad, relu=True, **kw)
                conv(t2, c3.w, c3.b, t1, n, h, w, c3.cin, c3.cout, c3.k, c3.stride, c3.pad, relu=False, add=cur, **kw)   # net(x) + x
                cur = t1
            else:
                conv(cur, L.w, L.b, self.logits, n, h, w, L.cin, L.cout, L.k, L.stride, L.pad, relu=False, out_padded=False, **kw)
        return h, w

    @torch.no_grad()
    def get_codebook_indices(self, images):
        """images f32 [B, C, H, W] on the GPU -> i64 [B, h*w] token ids."""
        ops = self.ops
        assert images.is_cuda and images.dtype == torch.float32 and images.shape[-2:] == (self.H, self.W)
        images = images.contiguous()
        B = images.shape[0]
        self._alloc(B)
        ops.nchw_to_padded_nhwc4(images, self.x0, *(self.norm or (None, None)))
        h, w = self._walk(B)
        M, hw = B * h * w, h * w
        if not self.certify:
            ops.argmax_rows(self.logits, M, self.num_tokens, self.ids, self.gap)
            return self.ids[:M].view(B, hw).clone()
        # ---- certification: margins on the device, flagged samples recomputed in fp32 (no host synchronisation)
        ops.argmax_rows(self.logits, M, self.num_tokens, self.ids, self.gap, rms=self.rms)
        ops.tok_flag_samples(self.gap, self.rms, B, hw, self.kappa, self.flag_list, self.flag_count, self.cert_stats)
        ex = self._exact
        R = ex.max_batch
        for off in range(0, B, R):                   # ceil(B / R) rounds cover ANY number of flagged samples
            ex._forward_dyn(images, self.norm, self.flag_list, self.flag_count, off, self.n_round)
            ops.tok_scatter_ids(ex.ids, self.flag_list, self.n_round, off, R, hw, self.ids)
        out = self.ids[:M].view(B, hw).clone()
        # run-time audit of the certification claim: one sample of every audit_every-th call is recomputed by the fp32 kernels
        # (whether it was flagged or not) and label mismatches are counted on the device -- no host synchronisation
        self._calls += 1
        if self.audit_every > 0 and self._calls % self.audit_every == 0:
            i = (self._calls // self.audit_every * 7) % B
            ids32 = ex.get_codebook_indices(images[i:i + 1])
            self.cert_stats[2] += (ids32.view(-1) != out[i]).sum()
            self.cert_stats[3] += 1
        return out

    def _forward_dyn(self, images, norm, lst, count, off, n_round):
        """fp32 path on the samples lst[off : off + min(capacity, count - off)] of `images` (count on the device): every launch
        covers the capacity and returns at once behind the live rows; ids of the live slots land in self.ids[: live * hw]."""
        ops = self.ops
        assert self.precision == "fp32"
        R = self.max_batch
        ops.tok_gather_images(images, norm[0] if norm else None, norm[1] if norm else None, lst, count, off, R, self.x0, n_round)
        h, w = self._walk(R, n_active=n_round)
        ops.argmax_rows(self.logits, R * h * w, self.num_tokens, self.ids, self.gap, n_samples=n_round, rows_per_sample=h * w)

    def certification_stats(self):
        """(flagged samples, calls) since construction -- one device->host read; for logs and the bench line."""
        if not self.certify:
            return None
        f, c, bad, aud = self.cert_stats.tolist()
        return {"flagged_samples": int(f), "calls": int(c), "kappa": self.kappa, "exact_capacity": self._exact.max_batch,
                "calibration": getattr(self, "calibration", None), "audited_samples": int(aud), "audit_mismatches": int(bad)}

    def last_top2_gap(self, B):
        """fp32 mode: best-minus-runner-up logit of every token of the last call (f32 [B, h*w]) -- how far each label
        is from flipping under a different fp32 summation order."""
        h, w = self.hw_out
        return self.gap[: B * h * w].view(B, h * w).clone()

    # ---------------------------------------------------------------- decoder (bf16; vae_model.py:160-171)
    def _pack_dec(self, conv, cin_pad=None, cout_pad=None):
        """A Conv2d of the decoder as a bf16 ConvLayer, channel counts zero-padded to cin_pad / cout_pad."""
        w = conv.weight.detach().float()                   # [Cout, Cin, k, k]
        co, ci, k, _ = w.shape
        cip, cop = cin_pad or ci, cout_pad or co
        w = F.pad(w.permute(0, 2, 3, 1), (0, cip - ci, 0, 0, 0, 0, 0, cop - co))
        b = conv.bias.detach().float() if conv.bias is not None else torch.zeros(co, device=w.device)
        return ConvLayer(w.reshape(cop, k * k * cip).to(torch.bfloat16).contiguous(), F.pad(b, (0, cop - co)).contiguous(),
                         cip, cop, k, conv.stride[0], conv.padding[0])

    def _decode_init(self):
        """Pack the decoder once: the codebook as a bf16 table with its dim padded to a multiple of 64, then in order
        ("conv1", ConvLayer) the 1x1 behind the codebook, ("res", (ConvLayer,) * 3), ("convt", ConvLayer with the phase-packed
        weight) and ("head", ConvLayer) = the final 1x1 with its output channels padded to 8."""
        vae = self._model
        cb = vae.codebook.weight.detach().float()
        cpad = -(-cb.shape[1] // 64) * 64
        d = {"table": F.pad(cb, (0, cpad - cb.shape[1])).to(torch.bfloat16).contiguous(), "cpad": cpad, "layers": [], "n": 0}
        cin = cpad                                         # channels (padded) the next layer reads
        for m in vae.decoder:
            if isinstance(m, nn.Sequential):               # ConvTranspose2d(4, s2, p1) + ReLU
                ct = m[0]
                assert ct.kernel_size == (4, 4) and ct.stride == (2, 2) and ct.padding == (1, 1)
                w = pack_convt_weight(ct.weight.detach().float(), cin_pad=cin).to(torch.bfloat16).contiguous()
                d["layers"].append(("convt", ConvLayer(w, ct.bias.detach().float().contiguous(), cin, ct.out_channels, 4, 2, 1)))
                cin = ct.out_channels
            elif isinstance(m, ResBlock):
                d["layers"].append(("res", tuple(self._pack_dec(m.net[i]) for i in (0, 2, 4))))
            elif m is vae.decoder[-1]:                     # final Conv2d(hidden, channels, 1)
                d["channels"] = m.out_channels
                d["layers"].append(("head", self._pack_dec(m, cout_pad=-(-m.out_channels // 8) * 8)))
            else:                                          # Conv2d(codebook_dim, hidden, 1) in front of the ResBlocks
                d["layers"].append(("conv1", self._pack_dec(m, cin_pad=cin)))
                cin = m.out_channels
        self._dec = d

    def _decode_alloc(self, n):
        """Zero-bordered bf16 buffers for chunks of n samples: the codebook level, three at the ResBlocks' level, one per
        transposed layer, and the dense head output."""
        d = self._dec
        if n <= d["n"]:
            return
        dev, bf = self.dev, torch.bfloat16
        h, w = self.hw_out
        d["n"], d["x0"], d["bufs"] = n, torch.zeros((n, h + 2, w + 2, d["cpad"]), dtype=bf, device=dev), {}
        for kind, L in d["layers"]:
            if kind == "head":
                d["out"] = torch.empty((n * h * w, L.cout), dtype=bf, device=dev)
                continue
            if kind == "convt":
                h, w = 2 * h, 2 * w
            cout = L[0].cout if kind == "res" else L.cout
            pool = d["bufs"].setdefault((h, w, cout), [])
            while len(pool) < (3 if kind == "res" else 1):
                pool.append(torch.zeros((n, h + 2, w + 2, cout), dtype=bf, device=dev))

    def _decode_chunk(self, ids):
        d, ops = self._dec, self.ops
        conv = ops.conv2d_nhwc
        n = ids.shape[0]
        h, w = self.hw_out
        cur = d["x0"]
        cur[:n, 1:-1, 1:-1] = d["table"][ids].view(n, h, w, d["cpad"])
        for kind, L in d["layers"]:
            if kind == "conv1":
                out = d["bufs"][(h, w, L.cout)][0]
                conv(cur, L.w, L.b, out, n, h, w, L.cin, L.cout, 1, 1, 0, relu=False)
                cur = out
            elif kind == "res":
                c1, c2, c3 = L
                pool = d["bufs"][(h, w, c1.cout)]
                t1 = next(t for t in pool if t is not cur)
                t2 = next(t for t in pool if t is not cur and t is not t1)
                conv(cur, c1.w, c1.b, t1, n, h, w, c1.cin, c1.cout, c1.k, c1.stride, c1.pad, relu=True)
                conv(t1, c2.w, c2.b, t2, n, h, w, c2.cin, c2.cout, c2.k, c2.stride, c2.pad, relu=True)
                conv(t2, c3.w, c3.b, t1, n, h, w, c3.cin, c3.cout, c3.k, c3.stride, c3.pad, relu=False, add=cur)   # net(x) + x
                cur = t1
            elif kind == "convt":
                out = d["bufs"][(2 * h, 2 * w, L.cout)][0]
                ops.convt2d_nhwc(cur, L.w, L.b, out, n, h, w, L.cin, L.cout, relu=True)
                cur, h, w = out, 2 * h, 2 * w
            else:
                conv(cur, L.w, L.b, d["out"], n, h, w, L.cin, L.cout, 1, 1, 0, relu=False, out_padded=False)
        return d["out"][: n * h * w, : d["channels"]].view(n, h, w, d["channels"]).permute(0, 3, 1, 2).float()

    @torch.no_grad()
    def decode(self, ids, decode_batch=None):
        """`DiscreteVAE.decode`: ids i64 [B, h*w] on the GPU -> f32 [B, C, H, W], in chunks of decode_batch samples (default:
        the constructor's; every sample's result is independent of the chunking)."""
        h, w = self.hw_out
        assert ids.is_cuda and ids.dtype == torch.int64 and ids.dim() == 2 and ids.shape[1] == h * w
        if self._dec is None:
            self._decode_init()
        step = max(1, int(decode_batch or self.decode_batch))
        B = ids.shape[0]
        self._decode_alloc(min(step, max(B, 1)))
        out = torch.empty((B, self._dec["channels"], self.H, self.W), dtype=torch.float32, device=self.dev)
        for i in range(0, B, step):
            out[i:i + step] = self._decode_chunk(ids[i:i + step])
        return out

    @torch.no_grad()
    def reconstruct(self, images):
        """(ids, recon): `get_codebook_indices`, then `decode` (the hard reconstruction of vae_model.py:240-245)."""
        ids = self.get_codebook_indices(images)
        return ids, self.decode(ids)
