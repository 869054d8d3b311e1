"""The fused engines behind modeling_mae.MaskedAutoencoderViT: flat fp32 parameter / gradient buffers (the ViTEngine contract:
vit_engine.FlatParams) and the explicit forward / backward of the MAE model.

`MaeEngineF32` holds the ONE forward / backward skeleton (im2col, patch GEMM, encoder assemble, encoder blocks, norm,
decoder_embed, decoder assemble, decoder blocks, decoder_norm, decoder_pred, loss -- and its mirror) and the fp32 kernels
(csrc/fp32_path.hip).  `MaeEngineBF16` runs the same skeleton on the bf16 MFMA kernels.  A precision is the set of hooks the
skeleton calls: `_alloc` (its batch buffers), `_im2col`, `_linear` / `_ln_fwd` (Linear / LayerNorm forward outside the
blocks), `_linear_bwd_w` / `_linear_bwd_x` / `_ln_bwd` (their backward: bias + weight gradient, data gradient), `_blk_fwd` /
`_blk_bwd` (a timm Block) and `sync_weights`.
"""
from functools import partial

import numpy as np
import torch

from . import ops
from .vit_engine import FlatParams, _pad
from .vit_engine_f32 import wgrad_f32


class MaeEngineF32(FlatParams):
    """The MAE model on the fp32 kernels (parity mode) + everything both precisions share."""
    precision = "fp32"
    act_dtype = torch.float32           # Linear / LayerNorm outputs that feed a GEMM

    def __init__(self, model):
        self.model = model
        p0 = next(model.parameters())
        assert p0.is_cuda, "mem_amd runs on the GPU only: move the model to cuda first (no CPU fallback)"
        self.dev = p0.device
        pe = model.patch_embed
        self.C = pe.proj.weight.shape[1]
        self.ph, self.pw = pe.patch_size
        self.H, self.W = pe.img_size
        self.L = pe.num_patches
        self.T = self.L + 1
        self.D = model.embed_dim
        self.Dd = model.decoder_embed.weight.shape[0]
        self.Pp = model.decoder_pred.weight.shape[0]
        self.Kpe = self.C * self.ph * self.pw
        self.enc = dict(pre="blocks.", depth=len(model.blocks), D=self.D, heads=model.blocks[0].attn.num_heads,
                        hidden=model.blocks[0].mlp.fc1.weight.shape[0])
        self.dec = dict(pre="decoder_blocks.", depth=len(model.decoder_blocks), D=self.Dd,
                        heads=model.decoder_blocks[0].attn.num_heads, hidden=model.decoder_blocks[0].mlp.fc1.weight.shape[0])
        self.eps = float(model.norm.eps)
        named = {n: p for n, p in model.named_parameters() if p.requires_grad}     # (pos_embed / decoder_pos_embed stay outside)
        dec_names = [n for n in named if n.startswith("decoder") or n == "mask_token"]
        enc_names = [n for n in named if n not in set(dec_names)]
        self._pack_flat(named, model.no_weight_decay(), [("decoder", dec_names), ("encoder", enc_names)])   # backward order
        self.gn_ws = torch.zeros(1024, dtype=torch.float64, device=self.dev)
        self.gnorm = torch.zeros(1, dtype=torch.float32, device=self.dev)
        self.loss_acc = torch.zeros(2, dtype=torch.float32, device=self.dev)       # [loss, 0] (mlm_acc is 0 for MAE)
        self.scratch2 = torch.zeros(2, dtype=torch.float32, device=self.dev)
        self.grad_hook = None
        self.weights_dirty = True
        self.B = 0
        self.K = None
        self.wT = {}

    def Wm(self, name):          # fp32 master of a weight as an [out, in] matrix
        return self.P(name).view(self.named[name].shape[0], -1)

    def Gw(self, name):          # its gradient
        return self.G(name).view(self.named[name].shape[0], -1)

    def _lin_names(self):
        out = ["decoder_embed.weight", "decoder_pred.weight"]
        for spec in (self.enc, self.dec):
            for i in range(spec["depth"]):
                out += [f"{spec['pre']}{i}.{k}.weight" for k in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")]
        return out

    def sync_weights(self):
        for n in self._lin_names():
            w = self.Wm(n)
            if n not in self.wT:
                self.wT[n] = torch.empty((w.shape[1], w.shape[0]), dtype=torch.float32, device=self.dev)
            ops.f32_transpose(w, w.shape[0], w.shape[1], self.wT[n])
        self.weights_dirty = False

    # ------------------------------------------------------------------ batch buffers
    def ensure_batch(self, B, K):
        if B <= self.B and K == self.K:
            return
        dev, f, h = self.dev, torch.float32, self.act_dtype
        e = lambda *s, dt=f: torch.empty(s, dtype=dt, device=dev)   # noqa: E731
        L, T, D, Dd = self.L, self.T, self.D, self.Dd
        Me, Md = B * (K + 1), B * T                                 # encoder rows (kept tokens + cls), decoder rows
        self.patches, self.xe, self.dxe = e(B * L, self.Kpe, dt=h), e(B * L, D), e(B * L, D)
        self.latent, self.meanE, self.rstdE, self.dlat = e(Me, D, dt=h), e(Me), e(Me), e(Me, D, dt=h)
        self.yd, self.dyd = e(Me, Dd), e(Me, Dd)
        self.hdn, self.meanD, self.rstdD = e(Md, Dd, dt=h), e(Md), e(Md)
        self.pred, self.dpred = e(Md, self.Pp), e(Md, self.Pp)
        self.row_loss = e(B * L)
        self._alloc(B, K, Me, Md)
        self.B, self.K = B, K

    def _alloc(self, B, K, Me, Md):
        """ea / da (the activations and gradient scratch of the two block stacks) and the weight-gradient operands."""
        dev, f = self.dev, torch.float32
        e = lambda *s: torch.empty(s, dtype=f, device=dev)   # noqa: E731

        def acts(spec, M):
            Dm, Hd = spec["D"], spec["hidden"]
            return dict(x=[torch.zeros((M, Dm), dtype=f, device=dev) for _ in range(2 * spec["depth"] + 1)],
                        a=[dict(h1=e(M, Dm), qkv=e(M, 3 * Dm), ao=e(M, Dm), h2=e(M, Dm), hpre=e(M, Hd), a=e(M, Hd),
                                mean1=e(M), rstd1=e(M), mean2=e(M), rstd2=e(M)) for _ in range(spec["depth"])],
                        dx=torch.zeros((M, Dm), dtype=f, device=dev), dh=e(M, Dm), dbig=e(M, Hd), dqkv=e(M, 3 * Dm), dao=e(M, Dm))
        self.ea, self.da = acts(self.enc, Me), acts(self.dec, Md)
        Rp = _pad(max(Md, B * self.L), 32)
        wide = max(3 * self.D, self.enc["hidden"], 3 * self.Dd, self.dec["hidden"], self.Pp, self.Kpe)
        self._wgrad32 = partial(wgrad_f32, e(wide, Rp), e(wide, Rp))   # (the transposed operands of the product)

    # ---- generic timm Block (x = x + attn(norm1(x)); x = x + mlp(norm2(x)))
    def _blk_fwd(self, spec, acts, i, B, T):
        P, G = self.P, ops.f32_gemm_nt
        D, Hd, heads = spec["D"], spec["hidden"], spec["heads"]
        M = B * T
        pre = f"{spec['pre']}{i}."
        a = acts["a"][i]
        xin, xmid, xout = acts["x"][2 * i], acts["x"][2 * i + 1], acts["x"][2 * i + 2]
        scale = (D // heads) ** -0.5
        ops.f32_layernorm_fwd(xin, P(pre + "norm1.weight"), P(pre + "norm1.bias"), a["h1"], a["mean1"], a["rstd1"], M, D, eps=self.eps)
        G(a["h1"], self.Wm(pre + "attn.qkv.weight"), M, 3 * D, D, ops.EPI_BIAS_BF16, out0=a["qkv"], bias=P(pre + "attn.qkv.bias"),
          colscale=scale, colscale_n=D)
        ops.f32_attn_fwd(a["qkv"], B, T, D, heads, None, None, a["ao"])
        G(a["ao"], self.Wm(pre + "attn.proj.weight"), M, D, D, ops.EPI_RESIDUAL, bias=P(pre + "attn.proj.bias"), resid=xmid,
          aux=xin, ldaux=D, rows_per_sample=T)
        ops.f32_layernorm_fwd(xmid, P(pre + "norm2.weight"), P(pre + "norm2.bias"), a["h2"], a["mean2"], a["rstd2"], M, D, eps=self.eps)
        G(a["h2"], self.Wm(pre + "mlp.fc1.weight"), M, Hd, D, ops.EPI_BIAS_GELU, out0=a["hpre"], out1=a["a"], bias=P(pre + "mlp.fc1.bias"))
        G(a["a"], self.Wm(pre + "mlp.fc2.weight"), M, D, Hd, ops.EPI_RESIDUAL, bias=P(pre + "mlp.fc2.bias"), resid=xout, aux=xmid,
          ldaux=D, rows_per_sample=T)

    def _blk_bwd(self, spec, acts, i, B, T):
        P, Gr, G = self.P, self.G, ops.f32_gemm_nt
        D, Hd, heads = spec["D"], spec["hidden"], spec["heads"]
        M = B * T
        pre = f"{spec['pre']}{i}."
        a = acts["a"][i]
        xin, xmid = acts["x"][2 * i], acts["x"][2 * i + 1]
        dx, dh, dbig, dqkv, dao = acts["dx"], acts["dh"], acts["dbig"], acts["dqkv"], acts["dao"]
        scale = (D // heads) ** -0.5
        # MLP branch: the branch output gradient IS dx (no layer scale, no drop path)
        ops.f32_colsum(dx, M, D, Gr(pre + "mlp.fc2.bias"))
        G(dx, self.wT[pre + "mlp.fc2.weight"], M, Hd, D, ops.EPI_DGELU, out0=dbig, aux=a["hpre"], colsum=Gr(pre + "mlp.fc1.bias"))
        self._wgrad32(dx, a["a"], M, D, Hd, Gr(pre + "mlp.fc2.weight"))
        self._wgrad32(dbig, a["h2"], M, Hd, D, Gr(pre + "mlp.fc1.weight"))
        G(dbig, self.wT[pre + "mlp.fc1.weight"], M, D, Hd, ops.EPI_BIAS_BF16, out0=dh)
        ops.f32_layernorm_bwd(dh, xmid, P(pre + "norm2.weight"), a["mean2"], a["rstd2"], dx, Gr(pre + "norm2.weight"),
                              Gr(pre + "norm2.bias"), M, D, accumulate=True)
        # attention branch
        ops.f32_colsum(dx, M, D, Gr(pre + "attn.proj.bias"))
        G(dx, self.wT[pre + "attn.proj.weight"], M, D, D, ops.EPI_BIAS_BF16, out0=dao)
        self._wgrad32(dx, a["ao"], M, D, D, Gr(pre + "attn.proj.weight"))
        ops.f32_attn_bwd(a["qkv"], dao, B, T, D, heads, scale, None, None, dqkv, None)
        ops.f32_colsum(dqkv, M, 3 * D, Gr(pre + "attn.qkv.bias"))
        self._wgrad32(dqkv, a["h1"], M, 3 * D, D, Gr(pre + "attn.qkv.weight"))
        G(dqkv, self.wT[pre + "attn.qkv.weight"], M, D, 3 * D, ops.EPI_BIAS_BF16, out0=dh)
        ops.f32_layernorm_bwd(dh, xin, P(pre + "norm1.weight"), a["mean1"], a["rstd1"], dx, Gr(pre + "norm1.weight"),
                              Gr(pre + "norm1.bias"), M, D, accumulate=True)

    # ---- the hooks outside the blocks: name = "patch_embed.proj" / "decoder_embed" / "decoder_pred", y = x W^T + b with
    # x [M, K], W [N, K]
    def _im2col(self, imgs, B):
        ops.f32_im2col(imgs, B, self.C, self.H, self.W, self.ph, self.pw, self.patches)

    def _linear(self, name, x, M, N, K, y):
        ops.f32_gemm_nt(x, self.Wm(name + ".weight"), M, N, K, ops.EPI_BIAS_BF16, out0=y, bias=self.P(name + ".bias"))

    def _linear_bwd_w(self, name, dy, x, M, N, K):
        """Weight and bias gradient; -> dy as the data-gradient GEMM takes it."""
        self._wgrad32(dy, x, M, N, K, self.G(name + ".weight"))
        ops.f32_colsum(dy, M, N, self.G(name + ".bias"))
        return dy

    def _linear_bwd_x(self, name, dy, M, N, K, dx):
        ops.f32_gemm_nt(dy, self.wT[name + ".weight"], M, K, N, ops.EPI_BIAS_BF16, out0=dx)

    def _ln_fwd(self, *a, **k):
        ops.f32_layernorm_fwd(*a, **k)

    def _ln_bwd(self, *a, **k):
        ops.f32_layernorm_bwd(*a, **k)

    # ------------------------------------------------------------------ forward / backward (both precisions)
    def forward(self, imgs, ids_keep, ids_restore, mask):
        assert imgs.is_cuda and imgs.dtype == torch.float32 and imgs.is_contiguous()
        B = imgs.shape[0]
        assert tuple(imgs.shape[1:]) == (self.C, self.H, self.W), f"Input image size {tuple(imgs.shape)} doesn't match the model"
        K = ids_keep.shape[1]
        self.ensure_batch(B, K)
        if self.weights_dirty:
            self.sync_weights()
        P, m = self.P, self.model
        L, T, D, Dd = self.L, self.T, self.D, self.Dd
        Me, Md = B * (K + 1), B * T
        self.cur = dict(B=B, K=K, ids_keep=ids_keep, ids_restore=ids_restore, mask=mask, imgs=imgs)
        self._im2col(imgs, B)
        self._linear("patch_embed.proj", self.patches, B * L, D, self.Kpe, self.xe)
        ops.mae_enc_assemble(self.xe, m.pos_embed.data.view(T, D), P("cls_token"), ids_keep, B, L, K, D, self.ea["x"][0])
        for i in range(self.enc["depth"]):
            self._blk_fwd(self.enc, self.ea, i, B, K + 1)
        self._ln_fwd(self.ea["x"][-1], P("norm.weight"), P("norm.bias"), self.latent, self.meanE, self.rstdE, Me, D, eps=self.eps)
        self._linear("decoder_embed", self.latent, Me, Dd, D, self.yd)
        ops.mae_dec_assemble(self.yd, P("mask_token"), m.decoder_pos_embed.data.view(T, Dd), ids_restore, B, L, K, Dd, self.da["x"][0])
        for i in range(self.dec["depth"]):
            self._blk_fwd(self.dec, self.da, i, B, T)
        self._ln_fwd(self.da["x"][-1], P("decoder_norm.weight"), P("decoder_norm.bias"), self.hdn, self.meanD, self.rstdD,
                     Md, Dd, eps=self.eps)
        self._linear("decoder_pred", self.hdn, Md, self.Pp, Dd, self.pred)
        ops.mae_loss(self.pred, imgs, mask, B, self.C, self.H, self.W, self.ph, m.LOSS_ONLY_MASKED_MAE, self.row_loss, self.dpred,
                     self.scratch2)
        self.loss_acc[0:1].copy_(self.scratch2[1:2])
        return self.loss_acc

    def backward(self):
        c = self.cur
        B, K = c["B"], c["K"]
        P, Gr = self.P, self.G
        L, T, D, Dd = self.L, self.T, self.D, self.Dd
        Me, Md = B * (K + 1), B * T
        self.attach_grads()
        self.flat_g.zero_()
        dy = self._linear_bwd_w("decoder_pred", self.dpred, self.hdn, Md, self.Pp, Dd)
        self._linear_bwd_x("decoder_pred", dy, Md, self.Pp, Dd, self.da["dh"])
        self._ln_bwd(self.da["dh"], self.da["x"][-1], P("decoder_norm.weight"), self.meanD, self.rstdD, self.da["dx"],
                     Gr("decoder_norm.weight"), Gr("decoder_norm.bias"), Md, Dd, accumulate=False)
        for i in reversed(range(self.dec["depth"])):
            self._blk_bwd(self.dec, self.da, i, B, T)
        ops.mae_dec_assemble_bwd(self.da["dx"], c["ids_restore"], B, L, K, Dd, self.dyd, Gr("mask_token"))
        dy = self._linear_bwd_w("decoder_embed", self.dyd, self.latent, Me, Dd, D)
        if self.grad_hook:
            self.grad_hook(0)                                         # the decoder bucket is final
        self._linear_bwd_x("decoder_embed", dy, Me, Dd, D, self.dlat)
        self._ln_bwd(self.dlat, self.ea["x"][-1], P("norm.weight"), self.meanE, self.rstdE, self.ea["dx"],
                     Gr("norm.weight"), Gr("norm.bias"), Me, D, accumulate=False)
        for i in reversed(range(self.enc["depth"])):
            self._blk_bwd(self.enc, self.ea, i, B, K + 1)
        ops.mae_enc_assemble_bwd(self.ea["dx"], c["ids_keep"], B, L, K, D, self.dxe, Gr("cls_token"))
        self._linear_bwd_w("patch_embed.proj", self.dxe, self.patches, B * L, D, self.Kpe)
        if self.grad_hook:
            self.grad_hook(1)

    # ------------------------------------------------------------------ optimizer primitives (ViTEngine contract)
    def grad_norm(self):
        ops.grad_norm(self.flat_g, self.nflat, self.gnorm, self.gn_ws)
        return self.gnorm

    def adamw_step(self, m, v, lr, wd, step, betas=(0.9, 0.95), eps=1e-8, max_norm=0.0):
        ops.adamw(self.flat_p, self.flat_g, m, v, self.nflat, self.wd_flags, lr, betas[0], betas[1], eps, wd, step,
                  gnorm=self.gnorm, max_norm=max_norm or 0.0)
        self.weights_dirty = True


class MaeEngineBF16(MaeEngineF32):
    """The MAE model on the bf16 MFMA kernels (same flat fp32 master buffers, optimizer and reducer contract as
    MaeEngineF32).  Rounding points = the reference under autocast (mem/engine_for_pretraining.py:141-149): every Linear /
    Conv output is bf16 (fp32 accumulate + fp32 bias), the residual stream, LayerNorm, softmax and the loss are fp32.

    32-wide heads (the decoder: 512 / 16): the attention kernels are built for 64-wide heads, so q / k / v of head h live
    in columns [64 h, 64 h + 32) of a padded [*, 3 * 64 * heads] qkv matrix and the other 32 columns are zero.  The qkv
    and proj weights have padded bf16 shadows (zero rows / columns), so the GEMMs produce and consume the padded layout
    directly; q k^T, the softmax and the real output columns are unchanged, the padded columns of every activation and
    gradient are exact zeros, and the weight gradients of the padded rows / columns (zero) are dropped when the real rows
    are copied back."""
    precision = "bf16"
    act_dtype = torch.bfloat16
    CS_COPIES = 8
    # LayerNorm backward fused with the following branch backward (the ViT engine's ln_bwd_branch kernel); False: the two-kernel
    # form (tests/test_mae_gpu.py holds both to the same golden)
    FUSE_LN_BRANCH = True

    def __init__(self, model):
        super().__init__(model)
        for spec in (self.enc, self.dec):
            hd = spec["D"] // spec["heads"]
            assert hd in (32, 64) and spec["D"] % 64 == 0 and spec["hidden"] % 64 == 0, \
                "bf16 MAE engine: head_dim 32 or 64, widths multiples of 64 (use precision='fp32' otherwise)"
            spec["hd"], spec["Dp"] = hd, spec["heads"] * 64
        assert self.Kpe % 64 == 0 and self.Pp % 8 == 0
        self.w16, self.wT16, self.bpad = {}, {}, {}
        self.set_gelu_dg(True)

    def set_gelu_dg(self, on):
        """fc1 keeps gelu'(h) (fp16) for the backward instead of the pre-activation (vit_engine.ViTEngine.set_gelu_dg)."""
        self.epi_gelu, self.epi_dgelu = (ops.EPI_BIAS_GELU_DG, ops.EPI_MUL_AUX) if on else (ops.EPI_BIAS_GELU, ops.EPI_DGELU)

    # ---- bf16 shadows of the Linear weights ([out,in] for forward, [in,out] for dgrad), padded where heads are 32 wide
    def _build_shadows(self):
        """Once: the bf16 twin of the whole flat master buffer ([out,in] shadows of unpadded weights are views of it), the
        padded fp32 staging matrices (zero outside the real rows / columns, which every sync overwrites), their bf16
        shadows, and the descriptors of ONE batched transpose launch for all [in,out]-major copies."""
        dev = self.dev
        self.flat_w16 = torch.zeros(self.nflat, dtype=torch.bfloat16, device=dev)
        self.pad_src, self.pad_cast, items = [], [], []   # pad_src: (staging fp32, view of its real part, fp32 master view)

        def add(name, src32, o, i, w16):
            self.w16[name] = w16
            self.wT16[name] = torch.empty((i, o), dtype=torch.bfloat16, device=dev)
            items.append((src32, o, i, self.wT16[name]))

        def plain(name):
            W = self.Wm(name)
            o, i = W.shape
            off, k = self.segs[name]
            add(name, W, o, i, self.flat_w16[off:off + k].view(o, i))
        plain("patch_embed.proj.weight"); plain("decoder_embed.weight"); plain("decoder_pred.weight")
        for spec in (self.enc, self.dec):
            H, D, Dp = spec["heads"], spec["D"], spec["Dp"]
            for i in range(spec["depth"]):
                pre = f"{spec['pre']}{i}."
                plain(pre + "mlp.fc1.weight"); plain(pre + "mlp.fc2.weight")
                if spec["hd"] == 64:
                    plain(pre + "attn.qkv.weight"); plain(pre + "attn.proj.weight")
                    continue
                Wq = torch.zeros((3 * Dp, D), dtype=torch.float32, device=dev)
                Wp = torch.zeros((D, Dp), dtype=torch.float32, device=dev)
                b = torch.zeros(3 * Dp, dtype=torch.float32, device=dev)
                self.pad_src += [(Wq, Wq.view(3, H, 64, D)[:, :, :32, :], self.Wm(pre + "attn.qkv.weight").view(3, H, 32, D)),
                                 (Wp, Wp.view(D, H, 64)[:, :, :32], self.Wm(pre + "attn.proj.weight").view(D, H, 32)),
                                 (None, b.view(3, H, 64)[:, :, :32], self.P(pre + "attn.qkv.bias").view(3, H, 32))]
                self.bpad[pre] = b
                add(pre + "attn.qkv.weight", Wq, 3 * Dp, D, torch.empty((3 * Dp, D), dtype=torch.bfloat16, device=dev))
                add(pre + "attn.proj.weight", Wp, D, Dp, torch.empty((D, Dp), dtype=torch.bfloat16, device=dev))
                self.pad_cast += [(Wq, self.w16[pre + "attn.qkv.weight"]), (Wp, self.w16[pre + "attn.proj.weight"])]
        desc = np.zeros((len(items), 6), dtype=np.int64)
        prefix = np.zeros(len(items) + 1, dtype=np.int32)
        for k, (src, R, Cc, dst) in enumerate(items):
            desc[k] = (src.data_ptr(), src.stride(0), R, Cc, dst.data_ptr(), dst.stride(0))
            prefix[k + 1] = prefix[k] + ((R + 63) // 64) * ((Cc + 63) // 64)
        self._tdesc, self._tprefix = torch.from_numpy(desc).to(dev), torch.from_numpy(prefix).to(dev)
        self._tn, self._ttiles = len(items), int(prefix[-1])

    def sync_weights(self):
        """fp32 masters -> bf16 shadows: one flat cast, the padded matrices refreshed (copy of the real part + cast), one
        batched transpose launch for the [in,out]-major copies."""
        if not hasattr(self, "flat_w16"):
            self._build_shadows()
        ops.cast_f32_bf16(self.flat_p, self.flat_w16, self.nflat)
        for stage, real, master in self.pad_src:
            real.copy_(master)
        for stage, w in self.pad_cast:
            ops.cast_f32_bf16(stage, w, stage.numel())
        ops.transpose_cast_batched(self._tdesc, self._tprefix, self._tn, self._ttiles)
        self.weights_dirty = False

    def _alloc(self, B, K, Me, Md):
        """ea / da, the bf16 twins of the Linear outputs and output gradients outside the blocks (`_linear` / `_linear_bwd_w`),
        the column-sum accumulator copies and the split-K workspace of the weight-gradient GEMMs."""
        dev, f, h = self.dev, torch.float32, torch.bfloat16
        e = lambda *s: torch.empty(s, dtype=f, device=dev)      # noqa: E731
        e16 = lambda *s: torch.empty(s, dtype=h, device=dev)    # noqa: E731
        L, T, D, Dd = self.L, self.T, self.D, self.Dd

        def acts(spec, M, Tt):
            Dm, Hd, Dp, heads = spec["D"], spec["hidden"], spec["Dp"], spec["heads"]
            TP = ops.attn_tokens_padded(Tt)
            window = (14, 14) if Tt == 197 else (1, Tt - 1)      # no position bias: any window with Tt - 1 cells (zero table)
            nrd = (2 * window[0] - 1) * (2 * window[1] - 1) + 3
            return dict(x=[torch.zeros((M, Dm), dtype=f, device=dev) for _ in range(2 * spec["depth"] + 1)],
                        a=[dict(h1=e16(M, Dm), qkv=torch.zeros((M, 3 * Dp), dtype=h, device=dev), ao=e16(M, Dp), h2=e16(M, Dm),
                                hpre=e16(M, Hd), a=e16(M, Hd), mean1=e(M), rstd1=e(M), mean2=e(M), rstd2=e(M),
                                lse=e(B, heads, TP)) for _ in range(spec["depth"])],
                        dx=torch.zeros((M, Dm), dtype=f, device=dev), dy16=e16(M, Dm), dh=e16(M, Dm), dbig16=e16(M, Hd),
                        dqkv16=e16(M, 3 * Dp), dao16=e16(M, Dp), delta=e(2 * M + 4, heads),
                        window=window, table=torch.zeros((nrd, heads), dtype=f, device=dev),
                        gq=torch.zeros((3 * Dp, Dm), dtype=f, device=dev) if spec["hd"] == 32 else None,
                        gp=torch.zeros((Dm, Dp), dtype=f, device=dev) if spec["hd"] == 32 else None,
                        gb=torch.zeros(3 * Dp, dtype=f, device=dev) if spec["hd"] == 32 else None)
        self.ea, self.da = acts(self.enc, Me, K + 1), acts(self.dec, Md, T)
        self.cs_ws = torch.zeros(self.CS_COPIES * max(self.enc["hidden"], self.dec["hidden"], self.enc["Dp"], self.dec["Dp"]),
                                 dtype=f, device=dev)         # column-sum accumulator copies of the fused GEMM epilogues
        self.y16 = {"patch_embed.proj": e16(B * L, D), "decoder_embed": e16(Me, Dd), "decoder_pred": e16(Md, self.Pp)}
        self.dy16 = {"patch_embed.proj": e16(B * L, D), "decoder_embed": e16(Me, Dd), "decoder_pred": e16(Md, self.Pp)}
        need = 0
        for spec, M in ((self.enc, Me), (self.dec, Md)):
            for n_out, n_in in ((3 * spec["Dp"], spec["D"]), (spec["D"], spec["Dp"]), (spec["hidden"], spec["D"]),
                                (spec["D"], spec["hidden"])):
                need = max(need, ops.gemm_tn_workspace(M, n_out, n_in))
        need = max(need, ops.gemm_tn_workspace(Md, self.Pp, Dd), ops.gemm_tn_workspace(Me, Dd, D),
                   ops.gemm_tn_workspace(B * L, D, self.Kpe))
        self.tn_ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)

    # ---- timm Block on the bf16 kernels
    def _blk_fwd(self, spec, acts, i, B, T):
        P = self.P
        D, Hd, heads, Dp = spec["D"], spec["hidden"], spec["heads"], spec["Dp"]
        M = B * T
        pre = f"{spec['pre']}{i}."
        a = acts["a"][i]
        xin, xmid, xout = acts["x"][2 * i], acts["x"][2 * i + 1], acts["x"][2 * i + 2]
        scale = spec["hd"] ** -0.5
        qb = self.bpad[pre] if spec["hd"] == 32 else P(pre + "attn.qkv.bias")
        ops.layernorm_fwd(xin, P(pre + "norm1.weight"), P(pre + "norm1.bias"), a["h1"], a["mean1"], a["rstd1"], M, D, eps=self.eps)
        ops.gemm_nt(a["h1"], self.w16[pre + "attn.qkv.weight"], M, 3 * Dp, D, ops.EPI_BIAS_BF16, out0=a["qkv"], bias=qb,
                    colscale=scale, colscale_n=Dp)
        ops.attn_fwd(a["qkv"], B, T, Dp, heads, acts["table"], acts["window"], a["ao"], a["lse"])
        ops.gemm_nt(a["ao"], self.w16[pre + "attn.proj.weight"], M, D, Dp, ops.EPI_RESIDUAL, bias=P(pre + "attn.proj.bias"),
                    resid=xmid, aux=xin, ldaux=D, rows_per_sample=T)
        ops.layernorm_fwd(xmid, P(pre + "norm2.weight"), P(pre + "norm2.bias"), a["h2"], a["mean2"], a["rstd2"], M, D, eps=self.eps)
        # (round 4: fc1 stores gelu'(h) as fp16 instead of the pre-activation, the backward multiplies: ViTEngine.set_gelu_dg)
        ops.gemm_nt(a["h2"], self.w16[pre + "mlp.fc1.weight"], M, Hd, D, self.epi_gelu, out0=a["hpre"], out1=a["a"],
                    bias=P(pre + "mlp.fc1.bias"))
        ops.gemm_nt(a["a"], self.w16[pre + "mlp.fc2.weight"], M, D, Hd, ops.EPI_RESIDUAL, bias=P(pre + "mlp.fc2.bias"),
                    resid=xout, aux=xmid, ldaux=D, rows_per_sample=T)

    def _wgrad16(self, dY, X, R, n_out, n_in, out):
        ops.gemm_tn(dY, X, R, n_out, n_in, out, accumulate=True, workspace=self.tn_ws)

    def _blk_bwd(self, spec, acts, i, B, T):
        P, Gr, Gw = self.P, self.G, self.Gw
        D, Hd, heads, Dp = spec["D"], spec["hidden"], spec["heads"], spec["Dp"]
        M = B * T
        pre = f"{spec['pre']}{i}."
        a = acts["a"][i]
        xin, xmid = acts["x"][2 * i], acts["x"][2 * i + 1]
        dx, dy, dh, dbig, dqkv, dao = acts["dx"], acts["dy16"], acts["dh"], acts["dbig16"], acts["dqkv16"], acts["dao16"]
        scale = spec["hd"] ** -0.5
        pad = spec["hd"] == 32
        # MLP branch: the branch output gradient IS dx (no layer scale, no drop path); Linear grad_outputs are bf16.
        # dy = bf16(dx) + its column sums: for every block but the last of a stack this already came out of the fused norm1
        # backward of block i + 1 (below); FUSE_LN_BRANCH = False keeps the two-kernel form
        fuse = self.FUSE_LN_BRANCH and D <= 1024
        if i == spec["depth"] - 1 or not fuse:
            ops.branch_bwd(dx, None, None, dy, None, Gr(pre + "mlp.fc2.bias"), M, D)
        # (fused column sums go to CS_COPIES accumulator copies, folded by a tiny kernel: atomics on one address serialise)
        ops.gemm_nt(dy, self.wT16[pre + "mlp.fc2.weight"], M, Hd, D, self.epi_dgelu, out0=dbig, aux=a["hpre"],
                    colsum=self.cs_ws, colsum_copies=self.CS_COPIES)
        ops.colsum_fold(self.cs_ws, self.CS_COPIES, Hd, Gr(pre + "mlp.fc1.bias"))
        self._wgrad16(dy, a["a"], M, D, Hd, Gw(pre + "mlp.fc2.weight"))
        self._wgrad16(dbig, a["h2"], M, Hd, D, Gw(pre + "mlp.fc1.weight"))
        ops.gemm_nt(dbig, self.wT16[pre + "mlp.fc1.weight"], M, D, Hd, ops.EPI_BIAS_BF16, out0=dh)
        # norm2 backward into dx + the attention branch's dy = bf16(dx) and proj-bias column sums: one pass over dx
        if fuse:
            ops.layernorm_bwd_branch(dh, xmid, P(pre + "norm2.weight"), a["mean2"], a["rstd2"], dx, Gr(pre + "norm2.weight"),
                                     Gr(pre + "norm2.bias"), M, D, None, None, dy, None, Gr(pre + "attn.proj.bias"))
        else:
            ops.layernorm_bwd(dh, xmid, P(pre + "norm2.weight"), a["mean2"], a["rstd2"], dx, Gr(pre + "norm2.weight"),
                              Gr(pre + "norm2.bias"), M, D, accumulate=True)
            ops.branch_bwd(dx, None, None, dy, None, Gr(pre + "attn.proj.bias"), M, D)
        # qkv.bias gradient without a pass over dqkv: the v part is colsum(dao) (sum_k dV_k = sum_q dO_q: softmax rows sum to
        # one), fused into the GEMM that produces dao; the q part comes out of the attention backward kernel; the k part is
        # zero in real arithmetic (sum_k dS_qk = 0 for every query row) and is left at zero
        gb = acts["gb"] if pad else Gr(pre + "attn.qkv.bias")
        if pad:
            gb.zero_()
        ops.gemm_nt(dy, self.wT16[pre + "attn.proj.weight"], M, Dp, D, ops.EPI_BIAS_BF16, out0=dao, colsum=self.cs_ws,
                    colsum_copies=self.CS_COPIES)
        ops.colsum_fold(self.cs_ws, self.CS_COPIES, Dp, gb[2 * Dp:3 * Dp])
        if pad:
            acts["gp"].zero_()
            self._wgrad16(dy, a["ao"], M, D, Dp, acts["gp"])
            Gw(pre + "attn.proj.weight").view(D, heads, 32).add_(acts["gp"].view(D, heads, 64)[:, :, :32])
        else:
            self._wgrad16(dy, a["ao"], M, D, Dp, Gw(pre + "attn.proj.weight"))
        ops.attn_bwd(a["qkv"], dao, a["lse"], acts["delta"], acts["table"], acts["window"], B, T, Dp, heads, scale, dqkv, None,
                     dq_bias=gb[0:Dp], out=a["ao"])
        if pad:
            acts["gq"].zero_()
            self._wgrad16(dqkv, a["h1"], M, 3 * Dp, D, acts["gq"])
            Gr(pre + "attn.qkv.bias").view(3, heads, 32).add_(acts["gb"].view(3, heads, 64)[:, :, :32])
            Gw(pre + "attn.qkv.weight").view(3, heads, 32, D).add_(acts["gq"].view(3, heads, 64, D)[:, :, :32, :])
        else:
            self._wgrad16(dqkv, a["h1"], M, 3 * D, D, Gw(pre + "attn.qkv.weight"))
        ops.gemm_nt(dqkv, self.wT16[pre + "attn.qkv.weight"], M, D, 3 * Dp, ops.EPI_BIAS_BF16, out0=dh)
        if fuse and i > 0:        # norm1 backward of block i + the MLP branch's dy / fc2-bias column sums of block i - 1
            pb = f"{spec['pre']}{i - 1}."
            ops.layernorm_bwd_branch(dh, xin, P(pre + "norm1.weight"), a["mean1"], a["rstd1"], dx, Gr(pre + "norm1.weight"),
                                     Gr(pre + "norm1.bias"), M, D, None, None, dy, None, Gr(pb + "mlp.fc2.bias"))
        else:
            ops.layernorm_bwd(dh, xin, P(pre + "norm1.weight"), a["mean1"], a["rstd1"], dx, Gr(pre + "norm1.weight"),
                              Gr(pre + "norm1.bias"), M, D, accumulate=True)

    # ---- the hooks outside the blocks: every Linear output is bf16 (fp32 accumulate + fp32 bias), widened for the fp32 consumer
    def _im2col(self, imgs, B):
        ops.im2col(imgs, B, self.C, self.H, self.W, self.ph, self.pw, self.patches)

    def _linear(self, name, x, M, N, K, y):
        y16 = self.y16[name]
        ops.gemm_nt(x, self.w16[name + ".weight"], M, N, K, ops.EPI_BIAS_BF16, out0=y16, bias=self.P(name + ".bias"))
        y[:M].copy_(y16[:M])          # (type promotion: + fp32 pos_embed, (pred - target) ** 2 in fp32 on the bf16 prediction)

    def _linear_bwd_w(self, name, dy, x, M, N, K):
        dy16 = self.dy16[name]
        ops.branch_bwd(dy, None, None, dy16, None, self.G(name + ".bias"), M, N)      # bf16 grad_output + its column sums
        self._wgrad16(dy16, x, M, N, K, self.Gw(name + ".weight"))
        return dy16

    def _linear_bwd_x(self, name, dy, M, N, K, dx):
        ops.gemm_nt(dy, self.wT16[name + ".weight"], M, K, N, ops.EPI_BIAS_BF16, out0=dx)

    def _ln_fwd(self, *a, **k):
        ops.layernorm_fwd(*a, **k)

    def _ln_bwd(self, *a, **k):
        ops.layernorm_bwd(*a, **k)
