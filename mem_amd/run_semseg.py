"""Stage 4: semantic segmentation training and evaluation -- ``python -m mem_amd.run_semseg``.

Mirror of mem/semantic_segmentation/tools/train.py with the values of configs/mem/upernet/mem_224_160k.py,
configs/_base_/schedules/schedule_160k.py and configs/_base_/datasets/dsec.py as flag defaults.  mmcv's runner, hooks and
registries are not carried; what they decide is restated here:

  * model        ``SegModel(EvBEiT(img_size=512, out_indices=(8, 9, 10, 11)), UPerHead, FCNHead)``; the total loss is the sum of
                 the entries whose key contains ``loss`` (mmseg's ``_parse_losses``).
  * groups       ``layer_decay_groups``: LayerDecayOptimizerConstructor, literally
                 (mmcv_custom/layer_decay_optimizer_constructor.py).
  * optimizer    ``SegOptimizer``: AdamW, no clipping.  ``FlatAdamW`` updates the backbone's flat buffer (trunk and necks) through
                 ``memhip_adamw_groups``; torch's AdamW updates the heads' parameters, which are not in the engine's buffer.
                 One ``param_groups`` list, ``zero_grad``, ``step``, ``state_dict`` in torch's per-parameter layout.
  * schedule     ``poly_lr``: mmcv's ``poly`` policy with linear warmup, per group, by iteration.
  * loop         iteration based; a checkpoint ``{"meta": {"iter", ...}, "state_dict", "optimizer"}`` every
                 ``--checkpoint_interval`` iterations and at the end (``iter_<n>.pth``, mmseg's keys); an evaluation every
                 ``--eval_interval`` iterations and under ``--eval_only``: test pipeline -> ``encode_decode`` -> ``SegEvaluator`` ->
                 one JSON line.  The data chain is ``mem_amd.seg_data``.
  * loss         ``--class_weight`` (a comma list, or a JSON file holding a list or an object with a ``"class_weight"`` key, such as
                 ``tools/seg_class_weights.py`` prints) weights the classes in both heads' losses; ``--ohem_min_kept N`` with the
                 optional ``--ohem_thresh T`` puts an ``OHEMPixelSampler`` on the decode head, as mmseg's OHEM configs do (no
                 per-head OHEM flags).  Both are off by default, are recorded in the checkpoint's ``meta``, and with a sampler the
                 training record gains ``decode.n_kept``.

Single GPU.  Distributed training, launchers, deepspeed, ``--aug-test``, the ``slide`` test mode and ``cat_max_ratio < 1`` parse
and are refused by name."""
import argparse
import json
import math
import os
import time
from pathlib import Path

import numpy as np
import torch

from . import utils

VIT_SIZES = {"base": (768, 12), "small": (384, 6), "tiny": (192, 3)}        # mem_224_160k.py:22-30

# flag -> (the only value taken, why)
REFUSED = {
    "launcher": ("none", "distributed launchers are not carried: single GPU"),
    "distributed": (False, "multi-GPU training needs a SyncBN exchange this entrypoint does not set up: single GPU"),
    "world_size": (1, "multi-GPU training needs a SyncBN exchange this entrypoint does not set up: single GPU"),
    "gpus": (1, "single GPU"),
    "deepspeed": (False, "deepspeed is not carried"),
    "enable_deepspeed": (False, "deepspeed is not carried"),
    "aug_test": (False, "multi-scale / flip test-time augmentation is not mirrored"),
    "test_mode": ("whole", "sliding-window inference is not mirrored (the reference config sets mode='whole')"),
}


def add_model_data_flags(p):
    """The source, model and data flags, shared with ``mem_amd.infer_semseg``."""
    p.add_argument("--data_root", default="synthetic", help="folder with imgs/<split>, anns/<split>, labels.txt, or 'synthetic'")
    p.add_argument("--train_split", default="train")
    p.add_argument("--val_split", default="val")
    p.add_argument("--work_dir", default="")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--device", default="cuda")
    p.add_argument("--workers_per_gpu", default=8, type=int)
    p.add_argument("--synthetic_samples", default=32, type=int)
    p.add_argument("--synthetic_events", default=20000, type=int)
    # model (mem_224_160k.py)
    p.add_argument("--vit", default="base", choices=sorted(VIT_SIZES))
    p.add_argument("--embed_dim", default=0, type=int, help="0: from --vit")
    p.add_argument("--num_heads", default=0, type=int, help="0: from --vit")
    p.add_argument("--depth", default=12, type=int)
    p.add_argument("--out_indices", default=None, type=int, nargs=4, help="default: the last four blocks (8 9 10 11 at depth 12)")
    p.add_argument("--net_size", default=[512, 512], type=int, nargs=2)
    p.add_argument("--drop", default=0.1, type=float, help="drop_path_rate of the backbone and dropout_ratio of both heads")
    p.add_argument("--init_values", default=0.1, type=float)
    p.add_argument("--necks", default="fused", choices=["fused", "torch"])
    p.add_argument("--num_classes", default=11, type=int)
    p.add_argument("--decode_channels", default=512, type=int)
    p.add_argument("--aux_channels", default=256, type=int)
    p.add_argument("--pool_scales", default=[1, 2, 3, 6], type=int, nargs="+")
    p.add_argument("--aux_loss_weight", default=0.4, type=float)
    p.add_argument("--pretrained", default="", help="a stage-2 / stage-3 checkpoint for the backbone")
    # data (dsec.py)
    p.add_argument("--canvas", default=[440, 640], type=int, nargs=2)
    p.add_argument("--crop_size", default=[440, 640], type=int, nargs=2)
    p.add_argument("--ratio_range", default=[1.0, 1.01], type=float, nargs=2)
    p.add_argument("--slice_max_evs", default=180000, type=int)
    p.add_argument("--cat_max_ratio", default=1.0, type=float)
    p.add_argument("--samples_per_gpu", default=16, type=int)


def parse_class_weight(text, num_classes=None):
    """``--class_weight``: "1,2.5,0" or a path to a JSON list / a JSON object with a "class_weight" key -> [float] or None"""
    if text is None or text == "":
        return None
    if os.path.exists(text):
        with open(text) as f:
            data = json.load(f)
        if isinstance(data, dict):
            if "class_weight" not in data:
                raise ValueError(f"--class_weight {text}: a JSON object needs a \"class_weight\" key")
            data = data["class_weight"]
    else:
        try:
            data = [float(v) for v in text.split(",")]
        except ValueError:
            raise ValueError(f"--class_weight {text!r}: neither a comma list of numbers nor an existing JSON file") from None
    if not isinstance(data, list) or not data or not all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in data):
        raise ValueError(f"--class_weight {text}: a non-empty list of numbers")
    weights = [float(v) for v in data]
    if any(not math.isfinite(v) or v < 0 for v in weights):
        raise ValueError(f"--class_weight {text}: weights must be finite and >= 0")
    if num_classes is not None and len(weights) != num_classes:
        raise ValueError(f"--class_weight names {len(weights)} weights, --num_classes is {num_classes}")
    return weights


def resolve_model_args(args):
    """The values that follow from others: the width and heads of --vit, the last four blocks."""
    dim, heads = VIT_SIZES[args.vit]
    args.embed_dim, args.num_heads = args.embed_dim or dim, args.num_heads or heads
    if args.out_indices is None:
        args.out_indices = list(range(args.depth - 4, args.depth))
    return args


def get_args(argv=None):
    p = argparse.ArgumentParser("mem_amd semantic segmentation (stage 4)", allow_abbrev=False)
    add_model_data_flags(p)
    # optimizer and schedule (mem_224_160k.py, schedule_160k.py)
    p.add_argument("--lr", default=5e-4, type=float)
    p.add_argument("--betas", default=[0.9, 0.999], type=float, nargs=2)
    p.add_argument("--weight_decay", default=0.05, type=float)
    p.add_argument("--layer_decay_rate", default=0.65, type=float)
    p.add_argument("--num_layers", default=0, type=int, help="paramwise_cfg.num_layers; 0: --depth")
    p.add_argument("--power", default=1.0, type=float)
    p.add_argument("--min_lr", default=0.0, type=float)
    p.add_argument("--warmup_iters", default=1500, type=int)
    p.add_argument("--warmup_ratio", default=1e-6, type=float)
    p.add_argument("--max_iters", default=160000, type=int)
    p.add_argument("--checkpoint_interval", default=4501, type=int)
    p.add_argument("--eval_interval", default=113, type=int)
    p.add_argument("--log_interval", default=50, type=int)
    p.add_argument("--resume", default="", help="a checkpoint of this entrypoint: iteration, optimizer and mask streams continue")
    p.add_argument("--eval_only", action="store_true")
    # the loss: class weights (both heads) and OHEM pixel sampling (decode head)
    p.add_argument("--class_weight", default="", help="comma list, or a JSON file: a list or an object with a class_weight key")
    p.add_argument("--ohem_min_kept", default=None, type=int, help="OHEMPixelSampler(min_kept=N) on the decode head; off when absent")
    p.add_argument("--ohem_thresh", default=None, type=float, help="its thresh; absent: the top-k mode")
    # parsed and refused
    p.add_argument("--launcher", default="none")
    p.add_argument("--distributed", action="store_true")
    p.add_argument("--world_size", default=1, type=int)
    p.add_argument("--gpus", default=1, type=int)
    p.add_argument("--local_rank", default=0, type=int)
    p.add_argument("--deepspeed", action="store_true")
    p.add_argument("--enable_deepspeed", action="store_true")
    p.add_argument("--aug-test", "--aug_test", dest="aug_test", action="store_true")
    p.add_argument("--test_mode", default="whole")
    args = p.parse_args(argv)
    for flag, (only, why) in REFUSED.items():
        if getattr(args, flag) != only:
            raise NotImplementedError(f"--{flag} {getattr(args, flag)}: {why}")
    if args.cat_max_ratio < 1.0:
        raise NotImplementedError(f"--cat_max_ratio {args.cat_max_ratio}: class-balanced crops are not mirrored (dsec.py sets 1.0)")
    resolve_model_args(args)
    args.num_layers = args.num_layers or args.depth
    args.class_weight = parse_class_weight(args.class_weight, args.num_classes)
    if args.ohem_thresh is not None and args.ohem_min_kept is None:
        raise ValueError("--ohem_thresh needs --ohem_min_kept")
    if args.ohem_min_kept is not None and args.ohem_min_kept < 0:
        raise ValueError(f"--ohem_min_kept {args.ohem_min_kept}: an integer >= 0")
    if args.ohem_thresh is not None and not 0.0 < args.ohem_thresh <= 1.0:
        raise ValueError(f"--ohem_thresh {args.ohem_thresh}: a probability in (0, 1]")
    return args


# ---------------------------------------------------------------------------------------------- model
def build_model(args):
    from .seg_heads import FCNHead, SegModel, UPerHead
    from .semseg_backbone import EvBEiT
    D = args.embed_dim
    backbone = EvBEiT(img_size=tuple(args.net_size), patch_size=16, embed_dim=D, depth=args.depth, num_heads=args.num_heads,
                      mlp_ratio=4, use_abs_pos_emb=False, use_rel_pos_bias=True, init_values=args.init_values,
                      drop_path_rate=args.drop, out_indices=tuple(args.out_indices), necks=args.necks)
    # the loss arguments: absent (the inference tool's flags) or off, both heads are built exactly as without them
    cw, min_kept = getattr(args, "class_weight", None), getattr(args, "ohem_min_kept", None)
    sampler = None if min_kept is None else dict(type="OHEMPixelSampler", thresh=getattr(args, "ohem_thresh", None), min_kept=min_kept)
    kw_decode, kw_aux = dict(loss_weight=1.0), dict(loss_weight=args.aux_loss_weight)
    if cw is not None or sampler is not None:
        kw_decode = dict(loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0, class_weight=cw, sampler=sampler))
    if cw is not None:
        kw_aux = dict(loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=args.aux_loss_weight, class_weight=cw))
    decode = UPerHead(in_channels=(D,) * 4, in_index=(0, 1, 2, 3), pool_scales=tuple(args.pool_scales), channels=args.decode_channels,
                      num_classes=args.num_classes, dropout_ratio=args.drop, align_corners=False, **kw_decode)
    aux = FCNHead(in_channels=D, in_index=2, channels=args.aux_channels, num_convs=1, concat_input=False, dropout_ratio=args.drop,
                  num_classes=args.num_classes, align_corners=False, **kw_aux)
    return SegModel(backbone, decode, aux)


def load_pretrained(backbone, path):
    """A stage-2 / stage-3 checkpoint into the backbone: the state dict under ``model`` / ``module`` / ``state_dict`` (or the
    file itself), the shared relative-position table expanded to every block, index buffers dropped, tables of another window
    resampled on the geometric grid, an absolute position embedding resized, then ``utils.load_state_dict`` (non-strict: it
    reports the keys of the classifier or the mask token it leaves out, and the necks it does not find)."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    for key in ("model", "module", "state_dict"):
        if isinstance(ckpt, dict) and key in ckpt:
            ckpt = ckpt[key]
            break
    ckpt = {(k[len("backbone."):] if k.startswith("backbone.") else k): v for k, v in ckpt.items()}
    own = backbone.state_dict()
    shared = "rel_pos_bias.relative_position_bias_table"
    if shared in ckpt:
        table = ckpt.pop(shared)
        for i in range(backbone.get_num_layers()):
            ckpt["blocks.%d.attn.relative_position_bias_table" % i] = table.clone()
    for key in [k for k in ckpt if "relative_position_index" in k]:
        ckpt.pop(key)
    ps = backbone.patch_embed.patch_shape
    for key in [k for k in ckpt if "relative_position_bias_table" in k and k in own]:
        src_n, dst_n = ckpt[key].shape[0], own[key].shape[0]
        extra = dst_n - (ps[0] * 2 - 1) * (ps[1] * 2 - 1)
        src, dst = int((src_n - extra) ** 0.5), int((dst_n - extra) ** 0.5)
        if src != dst:
            print("Position interpolate for %s from %dx%d to %dx%d" % (key, src, src, dst, dst))
            ckpt[key] = utils._resample_rel_pos_table(ckpt[key], src, dst, extra)
    if "pos_embed" in ckpt and backbone.pos_embed is not None:
        ckpt["pos_embed"] = utils._resize_pos_embed(ckpt["pos_embed"], backbone)
    utils.load_state_dict(backbone, ckpt)


# ---------------------------------------------------------------------------------------------- parameter groups
def get_num_layer_for_vit(var_name, num_max_layer):
    """layer_decay_optimizer_constructor.py:6-16, on the names of the whole segmentor (``backbone.`` prefix)."""
    if var_name in ("backbone.cls_token", "backbone.mask_token", "backbone.pos_embed"):
        return 0
    if var_name.startswith("backbone.patch_embed"):
        return 0
    if var_name.startswith("backbone.blocks"):
        return int(var_name.split(".")[2]) + 1
    return num_max_layer - 1


def layer_decay_groups(model, num_layers=12, layer_decay_rate=0.65, base_lr=5e-4, weight_decay=0.05):
    """LayerDecayOptimizerConstructor.add_params (layer_decay_optimizer_constructor.py:33-66), literally: ``num_layers + 2``
    layer ids, the embeddings 0, block i -> i + 1, everything else -- the necks ``backbone.fpn*`` and both heads -- the last;
    scale ``rate ** (num_layers + 2 - id - 1)``; no weight decay iff ``ndim == 1`` or the name ends in ``.bias``.  Its third
    clause, ``name in ('pos_embed', 'cls_token')``, never matches a name that carries the ``backbone.`` prefix, so those two
    3-d tensors DO decay: kept.  Groups appear in the order of their first parameter, with the reference's keys."""
    n = num_layers + 2
    groups = {}
    for name, param in model.named_parameters():
        if not param.requires_grad:
            continue
        if len(param.shape) == 1 or name.endswith(".bias") or name in ("pos_embed", "cls_token"):
            gname, wd = "no_decay", 0.0
        else:
            gname, wd = "decay", weight_decay
        layer_id = get_num_layer_for_vit(name, n)
        gname = "layer_%d_%s" % (layer_id, gname)
        if gname not in groups:
            scale = layer_decay_rate ** (n - layer_id - 1)
            groups[gname] = {"weight_decay": wd, "params": [], "param_names": [], "lr_scale": scale, "group_name": gname,
                             "lr": scale * base_lr}
        groups[gname]["params"].append(param)
        groups[gname]["param_names"].append(name)
    return list(groups.values())


# ---------------------------------------------------------------------------------------------- schedule
def poly_lr(base_lr, it, max_iters, power=1.0, min_lr=0.0, warmup_iters=1500, warmup_ratio=1e-6):
    """mmcv's PolyLrUpdaterHook with warmup='linear', by iteration (mmcv/runner/hooks/lr_updater.py): the regular value of
    iteration ``it``, scaled during the first ``warmup_iters`` iterations."""
    regular = (base_lr - min_lr) * (1.0 - it / max_iters) ** power + min_lr
    if it >= warmup_iters:
        return regular
    k = (1.0 - it / warmup_iters) * (1.0 - warmup_ratio)
    return regular * (1.0 - k)


def set_lr(optimizer, it, args):
    """every group from ITS base value (mmcv keeps it as ``initial_lr`` in the group, so it travels with the checkpoint)"""
    for g in optimizer.param_groups:
        g.setdefault("initial_lr", g["lr"])
        g["lr"] = poly_lr(g["initial_lr"], it, args.max_iters, args.power, args.min_lr, args.warmup_iters, args.warmup_ratio)


# ---------------------------------------------------------------------------------------------- optimizer
class SegOptimizer:
    """AdamW over the segmentor's parameter groups, in two halves behind one object: the parameters of ``model.backbone`` (trunk
    and necks) live in the engine's flat buffer and are updated by ``FlatAdamW`` (one ``memhip_adamw_groups`` launch); the
    heads' parameters are torch tensors of their own and are updated by ``torch.optim.AdamW``.  ``param_groups`` is the one
    list a schedule mutates: its ``lr`` / ``weight_decay`` are copied to both halves at every ``step``.  ``state_dict`` is
    torch's layout over that list (state index = position of the parameter in the concatenated groups)."""

    def __init__(self, model, param_groups, lr, betas=(0.9, 0.999), eps=1e-8):
        from .optim_factory import FlatAdamW
        self.param_groups = [dict(g) for g in param_groups]
        for g in self.param_groups:
            g.setdefault("lr", lr)
            g.setdefault("betas", tuple(betas))
            g.setdefault("eps", eps)
        inside = {id(p) for p in model.backbone.parameters()}
        self._has = []                                  # per group: (it has parameters in the flat half, in the torch half)
        flat_groups, head_groups = [], []
        for g in self.param_groups:
            pair = []
            for mine, dest in ((True, flat_groups), (False, head_groups)):
                ps = [p for p in g["params"] if (id(p) in inside) == mine]
                if ps:
                    dest.append({"params": ps, "lr": g["lr"], "weight_decay": g["weight_decay"]})
                pair.append(bool(ps))
            self._has.append(tuple(pair))
        self.flat = FlatAdamW(model.backbone, flat_groups, lr=lr, betas=betas, eps=eps) if flat_groups else None
        self.head = torch.optim.AdamW(head_groups, lr=lr, betas=tuple(betas), eps=eps) if head_groups else None

    def _push(self):
        """lr / weight_decay of every group to its part in each half (both halves keep their groups in this list's order;
        looked up per call: an optimizer replaces its group dicts when it loads a state)"""
        it_f = iter(self.flat.param_groups if self.flat else [])
        it_h = iter(self.head.param_groups if self.head else [])
        for g, (in_flat, in_head) in zip(self.param_groups, self._has):
            for sub in ([next(it_f)] if in_flat else []) + ([next(it_h)] if in_head else []):
                sub["lr"], sub["weight_decay"] = g["lr"], g["weight_decay"]

    def zero_grad(self, set_to_none=True):
        if self.flat is not None:
            self.flat.zero_grad()
        if self.head is not None:
            self.head.zero_grad(set_to_none=True)

    def step(self):
        self._push()
        if self.flat is not None:
            self.flat.step()
        if self.head is not None:
            self.head.step()

    def _per_param(self):
        """{id(param): its state} from both halves"""
        out = {}
        for opt in (self.flat, self.head):
            if opt is None:
                continue
            sd = opt.state_dict()
            params = [p for g in opt.param_groups for p in g["params"]]
            for idx, st in sd["state"].items():
                out[id(params[int(idx)])] = st
        return out

    def state_dict(self):
        per = self._per_param()
        state, groups, idx = {}, [], 0
        for g in self.param_groups:
            ids = []
            for p in g["params"]:
                if id(p) in per:
                    state[idx] = per[id(p)]
                ids.append(idx)
                idx += 1
            groups.append({**{k: v for k, v in g.items() if k != "params"}, "params": ids})
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        params = [p for g in self.param_groups for p in g["params"]]
        assert len(sd["param_groups"]) == len(self.param_groups) and sum(len(g["params"]) for g in sd["param_groups"]) == len(params), \
            "optimizer state of another model"
        for g, sg in zip(self.param_groups, sd["param_groups"]):
            g.update({k: v for k, v in sg.items() if k != "params"})
        by_param = {id(params[int(i)]): st for i, st in sd["state"].items()}
        for opt in (self.flat, self.head):
            if opt is None:
                continue
            own = opt.state_dict()
            mine = [p for g in opt.param_groups for p in g["params"]]
            own["state"] = {i: by_param[id(p)] for i, p in enumerate(mine) if id(p) in by_param}
            opt.load_state_dict(own)
        self._push()


# ---------------------------------------------------------------------------------------------- data
def build_pipeline(args):
    from .seg_data import SegBatchPipeline, SegPipelineConfig
    cfg = SegPipelineConfig(canvas=tuple(args.canvas), img_scale=tuple(args.canvas), ratio_range=tuple(args.ratio_range),
                            crop_size=tuple(args.crop_size), net_size=tuple(args.net_size), slice_max=args.slice_max_evs,
                            y_limit=args.canvas[0], cat_max_ratio=args.cat_max_ratio)
    return cfg, SegBatchPipeline(cfg, args.device)


def build_dataset(args, cfg, train):
    from .seg_data import EventSegDataset
    n = args.synthetic_samples if train else max(2, args.synthetic_samples // 4)
    return EventSegDataset(args.data_root, args.train_split if train else args.val_split, cfg, train=train, seed=args.seed,
                           n_synthetic=n, synthetic_events=args.synthetic_events, num_classes=args.num_classes)


def _loader(dataset, batch_sampler, workers):
    return torch.utils.data.DataLoader(dataset, batch_sampler=batch_sampler, num_workers=workers, collate_fn=dataset.collate,
                                       pin_memory=True, persistent_workers=False)


@torch.no_grad()
def evaluate(model, pipeline, dataset, args):
    """The test pipeline -> ``encode_decode`` -> ``SegEvaluator`` (whole-image: the logits are resized to the label's size
    there): ``{"aAcc", "mIoU", "mAcc", "IoU": {class: value}}``.  The labels are the files' own (the test pipeline leaves them
    alone); a sample's event slice is drawn with seed 0, so two evaluations of one model give the same figures."""
    from .seg_data import IterBatchSampler
    from .seg_loss import SegEvaluator
    was_training = model.training
    model.eval()
    ev = SegEvaluator(len(dataset.CLASSES))
    n = len(dataset)
    bs = args.samples_per_gpu
    batches = [[(i, 0) for i in range(s, min(s + bs, n))] for s in range(0, n, bs)]
    for events, offsets, labels, draws in _loader(dataset, batches, min(args.workers_per_gpu, len(batches))):
        img, _ = pipeline(events, offsets, None, draws, train=False)
        ev.update(model.encode_decode(img), labels.to(img.device))
    m = ev.compute()
    model.train(was_training)
    iou = [float(v) for v in m["IoU"]]
    return {"aAcc": m["aAcc"], "mIoU": m["mIoU"], "mAcc": m["mAcc"],
            "IoU": {c: (None if math.isnan(v) else v) for c, v in zip(dataset.CLASSES, iou)}}


# ---------------------------------------------------------------------------------------------- checkpoints
def save_checkpoint(path, model, optimizer, it, stream, args):
    """mmcv's layout: ``meta`` / ``state_dict`` / ``optimizer``; ``meta`` also carries the state of the mask stream (drop path
    and both heads' Dropout2d keys) and the run's seed."""
    meta = {"iter": it, "seed": args.seed, "drop_path_rng": stream.state(), "CLASSES": getattr(args, "CLASSES", None),
            "class_weight": getattr(args, "class_weight", None), "ohem_min_kept": getattr(args, "ohem_min_kept", None),
            "ohem_thresh": getattr(args, "ohem_thresh", None), "time": time.asctime()}
    tmp = str(path) + ".tmp"
    torch.save({"meta": meta, "state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()},
                "optimizer": optimizer.state_dict()}, tmp)
    os.replace(tmp, path)


def load_checkpoint(path, model, optimizer=None, stream=None):
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    model.load_state_dict(ckpt["state_dict"], strict=True)
    if getattr(model.backbone, "_engine", None) is not None:
        model.backbone._engine.weights_dirty = True
    if optimizer is not None and "optimizer" in ckpt:
        optimizer.load_state_dict(ckpt["optimizer"])
    if stream is not None and "drop_path_rng" in ckpt["meta"]:
        stream.load_state(ckpt["meta"]["drop_path_rng"])
    return int(ckpt["meta"]["iter"])


# ---------------------------------------------------------------------------------------------- main
def main(args):
    """Returns ``{"train": [log records], "eval": [evaluation records], "checkpoints": [paths], "iter": last iteration}``;
    every record is also printed as one JSON line."""
    from ._lib import require_gpu
    from .seg_data import IterBatchSampler
    require_gpu()
    utils.cap_host_threads(4)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    device = torch.device(args.device)
    work_dir = Path(args.work_dir) if args.work_dir else None
    if work_dir is not None:
        work_dir.mkdir(parents=True, exist_ok=True)
    cfg, pipeline = build_pipeline(args)
    model = build_model(args)
    if args.pretrained:
        load_pretrained(model.backbone, args.pretrained)
    model.to(device)
    model.backbone.engine                                 # packs the backbone's parameters into the flat buffers
    stream = model.backbone._dp_stream = utils.DropPathStream()
    stream.seed(args.seed)
    out = {"train": [], "eval": [], "checkpoints": [], "iter": 0}
    val = build_dataset(args, cfg, train=False)
    args.CLASSES = val.CLASSES
    if len(val.CLASSES) != args.num_classes:
        raise ValueError(f"labels.txt names {len(val.CLASSES)} classes, --num_classes is {args.num_classes}")

    def run_eval(it):
        rec = {"iter": it, **evaluate(model, pipeline, val, args)}
        print(json.dumps(rec), flush=True)
        out["eval"].append(rec)

    if args.eval_only:
        if not args.resume:
            raise ValueError("--eval_only needs --resume <checkpoint>")
        out["iter"] = load_checkpoint(args.resume, model)
        run_eval(out["iter"])
        return out
    groups = layer_decay_groups(model, args.num_layers, args.layer_decay_rate, args.lr, args.weight_decay)
    print("Param groups = %s" % json.dumps({g["group_name"]: {k: g[k] for k in ("param_names", "lr_scale", "lr", "weight_decay")}
                                            for g in groups}, indent=2))
    optimizer = SegOptimizer(model, groups, lr=args.lr, betas=tuple(args.betas))
    for g in optimizer.param_groups:
        g["initial_lr"] = g["lr"]
    start = 0
    if args.resume:
        start = load_checkpoint(args.resume, model, optimizer, stream)
        print("resumed from %s at iteration %d" % (args.resume, start))
    train = build_dataset(args, cfg, train=True)
    sampler = IterBatchSampler(len(train), args.samples_per_gpu, args.seed, start, args.max_iters)
    model.train()
    heads = [h for h in (model.decode_head, model.auxiliary_head) if h is not None]
    t0 = time.time()
    it = start
    for events, offsets, labels, draws in _loader(train, sampler, args.workers_per_gpu):
        set_lr(optimizer, it, args)
        img, label = pipeline(events, offsets, labels, draws, train=True)
        key = stream.key()                                # both heads' Dropout2d masks of this step (distinct sites)
        for h in heads:
            h.drop_key = key
        losses = model.forward_train(img, label)
        loss = sum(v.float() for k, v in losses.items() if "loss" in k)      # mmseg _parse_losses
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        it += 1
        if it % args.log_interval == 0 or it == args.max_iters:
            rec = {"iter": it, "lr": optimizer.param_groups[-1]["lr"], "loss": float(loss.detach()),
                   **{k: float(v.detach()) for k, v in losses.items()}, "time": round(time.time() - t0, 3)}
            if model.decode_head.loss_decode.sampler is not None:          # read where the loss is read: no other synchronisation
                rec["decode.n_kept"] = int(model.decode_head.loss_decode.last_stats["n_kept"])
            print(json.dumps(rec), flush=True)
            out["train"].append(rec)
        if work_dir is not None and (it % args.checkpoint_interval == 0 or it == args.max_iters):
            path = work_dir / ("iter_%d.pth" % it)
            save_checkpoint(path, model, optimizer, it, stream, args)
            out["checkpoints"].append(str(path))
        if it % args.eval_interval == 0:
            run_eval(it)
    out["iter"] = it
    out["lr"] = [g["lr"] for g in optimizer.param_groups]
    return out


if __name__ == "__main__":
    main(get_args())
