"""MAE variant of the pretraining model (`--mae 1`) -- mirror of /root/reference/mem/modeling_mae.py
(MaskedAutoencoderViT :101-302, factory mae_vit_base_patch16_dec512d8b :304-313; selected at
mem/run_mem_pretraining.py:231-232,275-276, loop branch mem/engine_for_pretraining.py:141-149).

Same constructor, parameter names / shapes (timm 0.4.12 PatchEmbed / Block / Attention / Mlp attribute names, so
reference checkpoints load), the same initialisation order (same torch seed -> same weights), fixed 2-D sin-cos position
embeddings, per-sample random masking by argsort of uniform noise, decoder with mask tokens, per-patch MSE loss.

Execution (``precision``):
  * "bf16" (default, what `--mae 1` trains with): `MaeEngineBF16` -- the reference's autocast placement on the bf16 MFMA
    kernels of the pretraining model (gemm_p8 / gemm_tn_p8 with fused bias / GELU / GELU' / residual epilogues, the
    LDS-resident attention kernels, LayerNorm, AdamW): bf16 GEMM / attention operands, fp32 accumulate, fp32 residual
    stream, LayerNorm statistics, softmax and loss.  The decoder's 32-wide heads run on the 64-wide attention kernels
    through zero-padded head slots (padded shadow weights: the padding columns are exact zeros end to end).
  * "fp32": `MaeEngineF32` on csrc/fp32_path.hip (fp32 MFMA GEMMs, generic attention with 64- and 32-wide heads) -- the
    parity mode (loss 2e-6 from the reference's fp32 run).
Both engines live in mem_amd/mae_engine.py (one forward / backward skeleton, per-precision hooks).  No CPU / eager fallback.
"""
from functools import partial

import numpy as np
import torch
import torch.nn as nn

from ._lib import require_gpu
from .mae_engine import MaeEngineBF16, MaeEngineF32

MASK_RATIO = 0.5


# ---- fixed sin-cos position embedding (modeling_mae.py:21-99)
def get_1d_sincos_pos_embed_from_grid(embed_dim, pos):
    assert embed_dim % 2 == 0
    omega = np.arange(embed_dim // 2, dtype=float)
    omega /= embed_dim / 2.0
    omega = 1.0 / 10000 ** omega
    out = np.einsum("m,d->md", pos.reshape(-1), omega)
    return np.concatenate([np.sin(out), np.cos(out)], axis=1)


def get_2d_sincos_pos_embed_from_grid(embed_dim, grid):
    assert embed_dim % 2 == 0
    return np.concatenate([get_1d_sincos_pos_embed_from_grid(embed_dim // 2, grid[0]),
                           get_1d_sincos_pos_embed_from_grid(embed_dim // 2, grid[1])], axis=1)


def get_2d_sincos_pos_embed(embed_dim, grid_size, cls_token=False):
    grid_h = np.arange(grid_size, dtype=np.float32)
    grid_w = np.arange(grid_size, dtype=np.float32)
    grid = np.stack(np.meshgrid(grid_w, grid_h), axis=0).reshape([2, 1, grid_size, grid_size])
    pos = get_2d_sincos_pos_embed_from_grid(embed_dim, grid)
    if cls_token:
        pos = np.concatenate([np.zeros([1, embed_dim]), pos], axis=0)
    return pos


# ---- parameter containers with timm 0.4.12's attribute names (construction order = the reference's RNG order)
class _Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, dim)
        self.drop = nn.Dropout(0.0)


class _Attention(nn.Module):
    def __init__(self, dim, num_heads):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=True)
        self.attn_drop = nn.Dropout(0.0)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(0.0)


class _Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio, norm_layer):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = _Attention(dim, num_heads)
        self.drop_path = nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio))


class _PatchEmbed(nn.Module):
    def __init__(self, img_size, patch_size, in_chans, embed_dim):
        super().__init__()
        img_size = (img_size, img_size) if isinstance(img_size, int) else tuple(img_size)
        patch_size = (patch_size, patch_size) if isinstance(patch_size, int) else tuple(patch_size)
        self.img_size, self.patch_size = img_size, patch_size
        self.grid_size = (img_size[0] // patch_size[0], img_size[1] // patch_size[1])
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)
        self.norm = nn.Identity()


class MaskedAutoencoderViT(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=1024, depth=24, num_heads=16,
                 decoder_embed_dim=512, decoder_depth=8, decoder_num_heads=16, mlp_ratio=4.0, norm_layer=nn.LayerNorm,
                 norm_pix_loss=False, LOSS_ONLY_MASKED_MAE=False):
        super().__init__()
        if norm_pix_loss:
            raise NotImplementedError("norm_pix_loss: the entrypoint builds the model with norm_pix_loss=0")
        self.patch_embed = _PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        num_patches = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, embed_dim), requires_grad=False)
        self.blocks = nn.ModuleList([_Block(embed_dim, num_heads, mlp_ratio, norm_layer) for _ in range(depth)])
        self.norm = norm_layer(embed_dim)
        self.decoder_embed = nn.Linear(embed_dim, decoder_embed_dim, bias=True)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, decoder_embed_dim))
        self.decoder_pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, decoder_embed_dim), requires_grad=False)
        self.decoder_blocks = nn.ModuleList([_Block(decoder_embed_dim, decoder_num_heads, mlp_ratio, norm_layer)
                                             for _ in range(decoder_depth)])
        self.decoder_norm = norm_layer(decoder_embed_dim)
        self.decoder_pred = nn.Linear(decoder_embed_dim, patch_size ** 2 * in_chans, bias=True)
        self.norm_pix_loss = norm_pix_loss
        self.LOSS_ONLY_MASKED_MAE = LOSS_ONLY_MASKED_MAE
        self.in_chans, self.embed_dim = in_chans, embed_dim
        print(f"LOSS_ONLY_MASKED_MAE = {self.LOSS_ONLY_MASKED_MAE}")
        self.initialize_weights()
        self._engine = None

    def initialize_weights(self):
        g = int(self.patch_embed.num_patches ** 0.5)
        self.pos_embed.data.copy_(torch.from_numpy(get_2d_sincos_pos_embed(self.pos_embed.shape[-1], g, True)).float().unsqueeze(0))
        self.decoder_pos_embed.data.copy_(
            torch.from_numpy(get_2d_sincos_pos_embed(self.decoder_pos_embed.shape[-1], g, True)).float().unsqueeze(0))
        w = self.patch_embed.proj.weight.data
        torch.nn.init.xavier_uniform_(w.view([w.shape[0], -1]))
        torch.nn.init.normal_(self.cls_token, std=0.02)
        torch.nn.init.normal_(self.mask_token, std=0.02)
        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            torch.nn.init.xavier_uniform_(m.weight)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def no_weight_decay(self):
        return set()

    # ------------------------------------------------------------------ helpers of the reference surface
    def patchify(self, imgs):
        p = self.patch_embed.patch_size[0]
        assert imgs.shape[2] == imgs.shape[3] and imgs.shape[2] % p == 0
        h = w = imgs.shape[2] // p
        c = imgs.shape[1]
        x = imgs.reshape(imgs.shape[0], c, h, p, w, p)
        return torch.einsum("nchpwq->nhwpqc", x).reshape(imgs.shape[0], h * w, p * p * c)

    def unpatchify(self, x):
        p = self.patch_embed.patch_size[0]
        h = w = int(x.shape[1] ** 0.5)
        c = x.shape[2] // (p * p)
        x = x.reshape(x.shape[0], h, w, p, p, c)
        return torch.einsum("nhwpqc->nchpwq", x).reshape(x.shape[0], c, h * p, h * p)

    @staticmethod
    def masking_indices(noise, mask_ratio):
        """random_masking (modeling_mae.py:204-231) without the gather: ids_keep, mask (0 keep / 1 remove), ids_restore."""
        N, L = noise.shape
        len_keep = int(L * (1 - mask_ratio))
        ids_shuffle = torch.argsort(noise, dim=1)
        ids_restore = torch.argsort(ids_shuffle, dim=1)
        ids_keep = ids_shuffle[:, :len_keep].contiguous()
        mask = torch.ones([N, L], device=noise.device)
        mask[:, :len_keep] = 0
        mask = torch.gather(mask, dim=1, index=ids_restore)
        return ids_keep, mask, ids_restore.contiguous()

    # ------------------------------------------------------------------ fused execution
    @property
    def engine(self):
        if self._engine is None:
            require_gpu()
            self._engine = MaeEngineF32(self) if getattr(self, "precision", "bf16") == "fp32" else MaeEngineBF16(self)
        return self._engine

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        if self._engine is not None:
            self._engine.weights_dirty = True
        return r

    def forward_loss(self, imgs, mask_ratio=MASK_RATIO, noise=None):
        """loss (device scalar tensor [1]) with everything kept for `backward()`; `noise` [N, L] overrides the draw."""
        eng = self.engine
        imgs = imgs.to(device=eng.dev, dtype=torch.float32).contiguous()
        if noise is None:
            noise = torch.rand(imgs.shape[0], eng.L, device=eng.dev)        # modeling_mae.py:213
        ids_keep, mask, ids_restore = self.masking_indices(noise.to(eng.dev), MASK_RATIO)   # the reference ignores mask_ratio (:295)
        eng.forward(imgs, ids_keep, ids_restore, mask.contiguous())
        self._last_mask = mask
        return eng.loss_acc

    def backward(self):
        self.engine.backward()

    def forward(self, imgs, mask_ratio=MASK_RATIO, noise=None):
        """-> (loss, unpatchify(pred), mask) like the reference (:294-298); inference surface (no autograd graph: training
        goes through forward_loss / backward)."""
        la = self.forward_loss(imgs, mask_ratio, noise)
        eng = self.engine
        B = imgs.shape[0]
        pred = eng.pred[: B * eng.T].view(B, eng.T, -1)[:, 1:, :].float()
        return la[0].clone(), self.unpatchify(pred.clone()), self._last_mask


def mae_vit_base_patch16_dec512d8b(norm_pix_loss=False, LOSS_ONLY_MASKED_MAE=False, precision="bf16", **kwargs):
    m = MaskedAutoencoderViT(patch_size=16, embed_dim=768, depth=12, num_heads=12, decoder_embed_dim=512,
                             decoder_depth=8, decoder_num_heads=16, mlp_ratio=4,
                             norm_layer=partial(nn.LayerNorm, eps=1e-6), norm_pix_loss=norm_pix_loss,
                             LOSS_ONLY_MASKED_MAE=LOSS_ONLY_MASKED_MAE, **kwargs)
    assert precision in ("bf16", "fp32")
    m.precision = precision
    return m

