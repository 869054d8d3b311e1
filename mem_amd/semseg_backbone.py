"""Segmentation backbone -- mirror of mem/semantic_segmentation/backbone/mem.py:277-452 (``EvBEiT``): the finetuning
trunk with four dense exits and the reference's feature-pyramid necks for patch size 16.

The trunk is ``ft_vit`` without its head (same parameter names, so a pretrained / finetuned checkpoint loads by key) and
runs in the fused HIP engine; the maps of the blocks ``out_indices`` leave it through ``VisionTransformer.forward_dense``
(``memhip_tokens_to_maps``), and in training their gradients enter the trunk backward at those depths
(``memhip_maps_to_tokens_add``).  The necks ``fpn1`` .. ``fpn4`` are torch modules (transposed convolutions, batch norm,
max pooling) with the reference's structure and state-dict keys (mem.py:331-346); their parameters live in the head bucket
of the engine's flat buffer, so the flat optimizer updates them with the trunk.  ``necks`` selects who computes ``fpn1`` and
``fpn2``: ``"torch"`` (default) the modules themselves, in fp32 on MIOpen; ``"fused"`` the HIP path of ``mem_amd/necks.py``
on the same parameters and buffers -- bf16 GEMMs of this library with fp32 accumulation, batch statistics / normalise /
GELU in fp32, the movement kernels of csrc/necks.hip around them, forward and backward.  A checkpoint moves freely between
the two.  ``fpn3`` (identity) and ``fpn4`` (max pooling) are torch's in both.

Not mirrored here: ``resize_in`` (feed the model its ``img_size``: ``mem_amd.seg_data`` fuses that resize into the data chain's
last kernel), the patch-8 necks, gradient checkpointing, the mmseg / mmcv registry and runner (``mem_amd.run_semseg`` restates
what they decide); the decode head ``UPerHead`` (and its pyramid branch alone, mmseg's ``PSPHead``), the auxiliary ``FCNHead``
and the thin ``EncoderDecoder`` are in ``mem_amd.seg_heads``, the heads' loss and metrics in ``mem_amd.seg_loss``.
"""
from functools import partial

import torch.nn as nn

from .modeling_finetune import VisionTransformer


class EvBEiT(VisionTransformer):
    _TAIL_PREFIXES = ("fpn",)                     # the torch tail behind the engine's trunk (ViTEngine: the head bucket)

    def __init__(self, img_size=(224, 224), patch_size=(16, 16), in_chans=3, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4.0, drop_rate=0.0, drop_path_rate=0.0, init_values=None, use_abs_pos_emb=True,
                 use_rel_pos_bias=False, use_shared_rel_pos_bias=False, out_indices=(3, 5, 7, 11), necks="torch", **kwargs):
        if necks not in ("torch", "fused"):
            raise ValueError(f'necks: "torch" or "fused", got {necks!r}')
        if "use_checkpoint" in kwargs:
            raise NotImplementedError("use_checkpoint: the fused engine keeps its own activation stash; gradient checkpointing "
                                      "is not part of it")
        if kwargs:
            raise TypeError(f"EvBEiT: unsupported arguments {sorted(kwargs)}")
        img_size = (img_size, img_size) if isinstance(img_size, int) else tuple(img_size)
        patch_size = (patch_size, patch_size) if isinstance(patch_size, int) else tuple(patch_size)
        if patch_size != (16, 16):
            raise NotImplementedError("EvBEiT: the necks of patch size 16 only (mem.py:332-346)")
        from .vit_engine import check_export
        out_indices = check_export(out_indices, depth, "out_indices")
        if len(out_indices) != 4:
            raise ValueError(f"out_indices: four block indices feed fpn1 .. fpn4, got {len(out_indices)}")
        super().__init__(img_size=img_size, patch_size=patch_size, in_chans=in_chans, num_classes=0, embed_dim=embed_dim,
                         depth=depth, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=True, drop_rate=drop_rate,
                         drop_path_rate=drop_path_rate, norm_layer=partial(nn.LayerNorm, eps=1e-6), init_values=init_values,
                         use_abs_pos_emb=use_abs_pos_emb, use_rel_pos_bias=use_rel_pos_bias,
                         use_shared_rel_pos_bias=use_shared_rel_pos_bias, use_mean_pooling=True)
        self._ctor_kwargs = dict(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim, depth=depth,
                                 num_heads=num_heads, mlp_ratio=mlp_ratio, drop_rate=drop_rate, drop_path_rate=drop_path_rate,
                                 init_values=init_values, use_abs_pos_emb=use_abs_pos_emb, use_rel_pos_bias=use_rel_pos_bias,
                                 use_shared_rel_pos_bias=use_shared_rel_pos_bias, out_indices=out_indices, necks=necks)
        self.necks = necks
        self._fused_necks = None                   # necks.FusedNecks, made on the first fused call (it needs the GPU library)
        self.fc_norm = None                        # no pooled head: the trunk ends at the last block's stream
        self.out_indices = out_indices
        self.fpn1 = nn.Sequential(nn.ConvTranspose2d(embed_dim, embed_dim, kernel_size=2, stride=2),
                                  nn.SyncBatchNorm(embed_dim), nn.GELU(),
                                  nn.ConvTranspose2d(embed_dim, embed_dim, kernel_size=2, stride=2))
        self.fpn2 = nn.Sequential(nn.ConvTranspose2d(embed_dim, embed_dim, kernel_size=2, stride=2))
        self.fpn3 = nn.Identity()
        self.fpn4 = nn.MaxPool2d(kernel_size=2, stride=2)

    def forward_features(self, x, drop_path_masks=None):
        """(fpn1(map_0), fpn2(map_1), fpn3(map_2), fpn4(map_3)): [B, D, 4Hp, 4Wp], [B, D, 2Hp, 2Wp], [B, D, Hp, Wp],
        [B, D, Hp/2, Wp/2] (mem.py:418-448)."""
        maps = self.forward_dense(x, self.out_indices, drop_path_masks)
        fpn1, fpn2 = self.fpn1, self.fpn2
        if self.necks == "fused":
            if self._fused_necks is None:
                from .necks import FusedNecks
                self._fused_necks = FusedNecks(self.fpn1, self.fpn2, engine=lambda: self.engine)
            fpn1, fpn2 = self._fused_necks.fpn1_apply, self._fused_necks.fpn2_apply
        return tuple(f(m) for f, m in zip((fpn1, fpn2, self.fpn3, self.fpn4), maps))

    def forward(self, x, drop_path_masks=None):
        return self.forward_features(x, drop_path_masks)
