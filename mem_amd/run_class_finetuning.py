"""Finetuning (stage 3) entrypoint -- mirror of mem/run_class_finetuning.py of the reference (get_args :68-274,
main :286-744): the same flag names and ``--config`` aliases (``class_batch_size``, ``class_dropout``, ...; unknown keys of
a shared .conf file are ignored like parse_known_args does), wired to pieces this package already has: ``ft_vit`` on the
fused engine, ``utils.finetune``, layer-wise lr decay, cosine schedules, ``mixup.Mixup``, the three-way criterion
(``loss.py``), ``utils.ModelEma``, ``engine_for_finetuning``.

    python -m mem_amd.run_class_finetuning --expweek 2026-10 --data_path synthetic --nb_classes 4 --input_H 64 --input_W 96 ...

Data: ``--data_set npy`` reads ``<data_path>/train|val/<class>/*.npy`` (label = index of the sorted class folder) through
the event transform chain; ``--data_path synthetic`` uses seeded synthetic event streams with ``label = index % nb_classes``.
``--freeze_backbone 1`` is the reference's linear-probing protocol: only ``head`` / ``fc_norm`` train and the engine runs
the trunk forward-only (no activation stash, no backward).  Flags of the reference that this path does not carry PARSE and then raise a one-line NotImplementedError naming the flag
when set away from the value that turns them off (``REFUSED``); nothing is silently ignored.  Three defaults therefore
differ from the reference's, whose own defaults select torchvision-side features: ``--aa`` (None instead of
rand-m9-mstd0.5-inc1), ``--reprob`` (0 instead of 0.25) and ``--num_workers`` (0: the event chain runs on the GPU in this
process).  ``--no_model_ema`` is an addition (the reference's ``--model_ema`` can only stay on).

Data parallel (``torchrun --nproc_per_node N -m mem_amd.run_class_finetuning ...``; the reference wraps the model in DDP,
mem/run_class_finetuning.py:559-565): ``parallel.attach_reducer`` broadcasts rank 0's weights BEFORE the EMA twin and the
optimizer are built and exchanges the gradient buckets from the engine's backward hook through a ``parallel.StepExchange``
(accumulation: on the update micro-step only; frozen trunk: the head bucket only).  ``--dist_eval`` shards the validation
set; only the main process writes checkpoints, ``log.txt`` and ``eval.txt``."""
import argparse
import datetime
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

from . import utils
from .parallel import attach_reducer
from .run_mem_pretraining import _config_file_args, ops_mod

# flag -> (value that turns it off, why it is refused)
REFUSED = {
    "enable_deepspeed": (False, "the deepspeed branch is not part of the fused path"),
    "linear_probe": (False, "the BatchNorm head it stands for (use_batch_norm) is not carried"),
    "attn_drop_rate": (0.0, "the fused attention kernels carry no dropout masks"),
    "model_ema_force_cpu": (False, "the EMA lives in the engine's flat device buffer; there is no CPU path"),
    "aa": (None, "torchvision / timm auto-augment belongs to the image dataset builders"),
    "reprob": (0.0, "random erasing belongs to the image dataset builders"),
    "MAE": (0, "finetuning the MAE variant is not carried"),
    "pretrained": (0, "downloads timm ImageNet weights"),
}
REFUSED_DATA_SETS = ("IMNET", "CIFAR", "image_folder", "dsec_semseg")


def _none_or_str(v):
    return None if v in ("None", "none", "") else v


def get_args(argv=None):
    p = argparse.ArgumentParser("Finetuning script", add_help=False, allow_abbrev=False)
    p.add_argument("--expweek", type=str, required=True)
    p.add_argument("--expname", default=None, type=str)
    p.add_argument("--batch_size", "--class_batch_size", default=64, type=int)
    p.add_argument("--epochs", "--class_epochs", default=30, type=int)
    p.add_argument("--update_freq", "--class_update_freq", default=1, type=int)
    p.add_argument("--save_ckpt_freq", "--class_save_ckpt_freq", default=5, type=int)
    # event preprocessing (shared with pretraining)
    p.add_argument("--timesurface", type=int, default=0)
    p.add_argument("--hotpixfilter", type=int, default=1)
    p.add_argument("--hotpix_num_stds", type=float, default=10)
    p.add_argument("--logtrafo", type=int, default=0)
    p.add_argument("--gammatrafo", type=int, default=0)
    p.add_argument("--gamma", type=float, default=0.5)
    p.add_argument("--normalize_events", type=int, default=1)
    p.add_argument("--slice_max_evs", type=int, default=30000)
    p.add_argument("--max_random_shift_evs", type=int, default=15)
    p.add_argument("--rand_aug", type=int, default=1)
    p.add_argument("--MAE", "--mae", default=0, type=int)
    p.add_argument("--freeze_backbone", default=0, type=int)
    p.add_argument("--linear_probe", action="store_true", default=False)
    p.add_argument("--num_layers", default=4, type=int)
    p.add_argument("--transformer_depth", default=12, type=int)
    p.add_argument("--transformer_heads", default=12, type=int)
    p.add_argument("--transformer_mlp_ratio", default=4, type=int)
    p.add_argument("--transformer_emb", default=768, type=int)
    # model
    p.add_argument("--model", default="ft_vit", type=str, metavar="MODEL")
    p.add_argument("--pretrained", default=0, type=int)
    p.add_argument("--rel_pos_bias", action="store_true")
    p.add_argument("--disable_rel_pos_bias", action="store_false", dest="rel_pos_bias")
    p.set_defaults(rel_pos_bias=True)
    p.add_argument("--abs_pos_emb", action="store_true")
    p.set_defaults(abs_pos_emb=False)
    p.add_argument("--layer_scale_init_value", default=0.1, type=float)
    p.add_argument("--input_H", default=128, type=int)
    p.add_argument("--input_W", default=128, type=int)
    p.add_argument("--input_size", default=224, type=int)
    p.add_argument("--drop", "--class_dropout", type=float, default=0.0, metavar="PCT")
    p.add_argument("--attn_drop_rate", type=float, default=0.0, metavar="PCT")
    p.add_argument("--drop_path", "--class_drop_path", type=float, default=0.1, metavar="PCT")
    p.add_argument("--disable_eval_during_finetuning", action="store_true", default=False)
    p.add_argument("--model_ema", action="store_true", default=True)
    p.add_argument("--no_model_ema", action="store_false", dest="model_ema")       # (the reference's flag can only stay on)
    p.add_argument("--model_ema_decay", type=float, default=0.9999)
    p.add_argument("--model_ema_force_cpu", action="store_true", default=False)
    # optimizer
    p.add_argument("--opt", default="adamw", type=str, metavar="OPTIMIZER")
    p.add_argument("--opt_eps", default=1e-8, type=float, metavar="EPSILON")
    p.add_argument("--opt_betas", default=None, type=float, nargs="+", metavar="BETA")
    p.add_argument("--clip_grad", type=float, default=None, metavar="NORM")
    p.add_argument("--momentum", type=float, default=0.9, metavar="M")
    p.add_argument("--weight_decay", "--class_weight_decay", type=float, default=0.3)
    p.add_argument("--weight_decay_end", type=float, default=None)
    p.add_argument("--lr", "--class_lr", type=float, default=5e-4, metavar="LR")
    p.add_argument("--layer_decay", "--class_layer_decay", type=float, default=0.9)
    p.add_argument("--warmup_lr", type=float, default=1e-6, metavar="LR")
    p.add_argument("--min_lr", type=float, default=1e-6, metavar="LR")
    p.add_argument("--warmup_epochs", "--class_warmup_epochs", type=int, default=5, metavar="N")
    p.add_argument("--warmup_steps", type=int, default=-1, metavar="N")
    # augmentation
    p.add_argument("--color_jitter", "--class_color_jitter", type=float, default=0.0, metavar="PCT")
    p.add_argument("--aa", type=_none_or_str, default=None, metavar="NAME")
    p.add_argument("--smoothing", type=float, default=0.1)
    p.add_argument("--train_interpolation", type=str, default="bicubic")
    p.add_argument("--crop_pct", type=float, default=None)
    p.add_argument("--reprob", type=float, default=0.0, metavar="PCT")
    p.add_argument("--remode", type=str, default="pixel")
    p.add_argument("--recount", type=int, default=1)
    p.add_argument("--resplit", action="store_true", default=False)
    p.add_argument("--mixup", type=float, default=0.8)
    p.add_argument("--cutmix", type=float, default=1.0)
    p.add_argument("--cutmix_minmax", type=float, nargs="+", default=None)
    p.add_argument("--mixup_prob", type=float, default=0.0)
    p.add_argument("--mixup_switch_prob", type=float, default=0.5)
    p.add_argument("--mixup_mode", type=str, default="batch")
    # finetuning
    p.add_argument("--finetune", default="")
    p.add_argument("--model_key", default="model|module", type=str)
    p.add_argument("--model_prefix", default="", type=str)
    p.add_argument("--init_scale", default=0.001, type=float)
    p.add_argument("--use_mean_pooling", action="store_true")
    p.set_defaults(use_mean_pooling=True)
    p.add_argument("--use_cls", action="store_false", dest="use_mean_pooling")
    p.add_argument("--disable_weight_decay_on_rel_pos_bias", action="store_true", default=False)
    # data
    p.add_argument("--data_path", default="synthetic", type=str)
    p.add_argument("--eval_data_path", default=None, type=str)
    p.add_argument("--nb_classes", default=0, type=int)
    p.add_argument("--imagenet_default_mean_and_std", default=False, action="store_true")
    p.add_argument("--resize", action="store_true", default=False)
    p.add_argument("--data_set", default="npy", choices=["CIFAR", "IMNET", "image_folder", "npy", "dsec_semseg"], type=str)
    p.add_argument("--synthetic_samples", default=64, type=int)
    p.add_argument("--canvas_max_H", default=0, type=int)
    p.add_argument("--canvas_max_W", default=0, type=int)
    p.add_argument("--output_dir", default="")
    p.add_argument("--log_dir", default="./logs")
    p.add_argument("--device", default="cuda")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--resume", default="")
    p.add_argument("--auto_resume", action="store_true")
    p.add_argument("--no_auto_resume", action="store_false", dest="auto_resume")
    p.set_defaults(auto_resume=True)
    p.add_argument("--save_ckpt", action="store_true")
    p.add_argument("--no_save_ckpt", action="store_false", dest="save_ckpt")
    p.set_defaults(save_ckpt=True)
    p.add_argument("--start_epoch", default=0, type=int, metavar="N")
    p.add_argument("--eval", action="store_true")
    p.add_argument("--dist_eval", action="store_true", default=False)
    p.add_argument("--num_workers", default=0, type=int)     # the event chain runs on the GPU: samples are made in this process
    p.add_argument("--pin_mem", action="store_true")
    p.add_argument("--no_pin_mem", action="store_false", dest="pin_mem")
    p.set_defaults(pin_mem=True)
    p.add_argument("--world_size", default=1, type=int)
    p.add_argument("--local_rank", default=-1, type=int)
    p.add_argument("--gpu", default=0, type=int)
    p.add_argument("--dist_on_itp", action="store_true")
    p.add_argument("--dist_url", default="env://")
    p.add_argument("--enable_deepspeed", action="store_true", default=False)
    p.add_argument("--wandb", type=int, default=0)
    argv = _config_file_args(list(sys.argv[1:] if argv is None else argv))
    args = p.parse_known_args(argv)[0]
    for flag, (off, why) in REFUSED.items():
        if getattr(args, flag) != off:
            raise NotImplementedError(f"--{flag} {getattr(args, flag)}: {why}")
    if args.data_set in REFUSED_DATA_SETS:
        raise NotImplementedError(f"--data_set {args.data_set}: the torchvision dataset builders are not carried (npy only)")
    if args.model not in ("ft_vit",):
        raise NotImplementedError(f"--model {args.model}: the finetuning model of this package is ft_vit")
    return args


class _LabelledEvents(torch.utils.data.Dataset):
    """(transform(events of sample i), label i): the per-sample surface of the event chain (datasets.TransformNPY)."""

    def __init__(self, source, labels, transform):
        self.source, self.labels, self.transform = source, labels, transform

    def __len__(self):
        return len(self.labels)

    def __getitem__(self, i):
        return self.transform(self.source(i)), int(self.labels[i])


def build_dataset(is_train, args):
    """(dataset, nb_classes): class sub-folders of .npy event files, or seeded synthetic streams."""
    from .datasets import NpyFolderSource, SyntheticEventSource, TransformNPY, _host_loader
    if args.data_path == "synthetic":
        assert args.nb_classes >= 2, "--data_path synthetic needs --nb_classes"
        args.fixed_canvas = True
        n = args.synthetic_samples if is_train else max(2, args.synthetic_samples // 4)
        src = SyntheticEventSource(min(args.slice_max_evs, 20000), args.input_W, args.input_H, seed=1234 if is_train else 4321)
        return _LabelledEvents(src, [i % args.nb_classes for i in range(n)], TransformNPY(is_train, args)), args.nb_classes
    base = args.data_path if is_train or not args.eval_data_path else args.eval_data_path
    root = next((os.path.join(base, d) for d in (("train", "extracted_train", "train_events") if is_train else
                                                 ("val", "extracted_val", "test_events"))
                 if os.path.isdir(os.path.join(base, d))), None)
    assert root is not None, f"{base}: no train / val folder of class sub-folders"
    src = NpyFolderSource(root, _host_loader(args))
    classes = sorted({os.path.basename(os.path.dirname(f)) for f in src.files})
    index = {c: i for i, c in enumerate(classes)}
    labels = [index[os.path.basename(os.path.dirname(f))] for f in src.files]
    return _LabelledEvents(src, labels, TransformNPY(is_train, args)), len(classes)


def get_model(args):
    from .modeling_finetune import ft_vit
    print(f"Creating model: {args.model}")
    return ft_vit(img_size=(args.input_H, args.input_W), patch_size=(2 ** args.num_layers, 2 ** args.num_layers),
                  embed_dim=args.transformer_emb, depth=args.transformer_depth, num_heads=args.transformer_heads,
                  mlp_ratio=args.transformer_mlp_ratio, num_classes=args.nb_classes, drop_rate=args.drop,
                  drop_path_rate=args.drop_path, attn_drop_rate=args.attn_drop_rate, use_mean_pooling=args.use_mean_pooling,
                  init_scale=args.init_scale, use_rel_pos_bias=args.rel_pos_bias, use_abs_pos_emb=args.abs_pos_emb,
                  init_values=args.layer_scale_init_value, in_chans=3)


def build_criterion(args, mixup_fn):
    """mem/run_class_finetuning.py:609-616."""
    from .loss import LabelSmoothingCrossEntropy, SoftTargetCrossEntropy
    if mixup_fn is not None:
        return SoftTargetCrossEntropy()               # smoothing is folded into the mixed targets
    if args.smoothing > 0.:
        return LabelSmoothingCrossEntropy(smoothing=args.smoothing)
    return torch.nn.CrossEntropyLoss()


def main(args):
    from .engine_for_finetuning import evaluate, train_one_epoch
    from .mixup import Mixup
    from .optim_factory import LayerDecayValueAssigner, create_optimizer
    utils.init_distributed_mode(args)
    utils.cap_host_threads(4)
    print(args)
    device = torch.device(args.device)
    seed = args.seed + utils.get_rank()
    torch.manual_seed(seed)
    np.random.seed(seed)
    dataset_train, args.nb_classes = build_dataset(True, args)
    dataset_val = None if args.disable_eval_during_finetuning else build_dataset(False, args)[0]
    num_tasks, rank = utils.get_world_size(), utils.get_rank()
    sampler_train = torch.utils.data.DistributedSampler(dataset_train, num_replicas=num_tasks, rank=rank, shuffle=True)
    loader_args = dict(num_workers=args.num_workers, pin_memory=args.pin_mem, drop_last=False)
    # (Mixup asserts an even batch, like timm: drop_last only when mixing, so that a ragged last batch cannot trip it)
    mixup_active = args.mixup > 0 or args.cutmix > 0. or args.cutmix_minmax is not None
    mixup_fn = None
    if mixup_active and args.mixup_prob != 0.0:
        print("Mixup is activated!")
        mixup_fn = Mixup(mixup_alpha=args.mixup, cutmix_alpha=args.cutmix, cutmix_minmax=args.cutmix_minmax,
                         prob=args.mixup_prob, switch_prob=args.mixup_switch_prob, mode=args.mixup_mode,
                         label_smoothing=args.smoothing, num_classes=args.nb_classes)
        loader_args["drop_last"] = True
    data_loader_train = torch.utils.data.DataLoader(dataset_train, sampler=sampler_train, batch_size=args.batch_size, **loader_args)
    data_loader_val = None
    if dataset_val is not None:
        if args.dist_eval:
            if len(dataset_val) % num_tasks != 0:
                print("Warning: Enabling distributed evaluation with an eval dataset not divisible by process number. "
                      "This will slightly alter validation results as extra duplicate entries are added to achieve "
                      "equal num of samples per-process.")
            sampler_val = torch.utils.data.DistributedSampler(dataset_val, num_replicas=num_tasks, rank=rank, shuffle=False)
        else:
            sampler_val = torch.utils.data.SequentialSampler(dataset_val)      # every rank evaluates the whole set
        data_loader_val = torch.utils.data.DataLoader(dataset_val, sampler=sampler_val,
                                                      batch_size=int(1.5 * args.batch_size), num_workers=args.num_workers,
                                                      pin_memory=args.pin_mem, drop_last=False)
    model = get_model(args)
    args.patch_size = model.patch_embed.patch_size
    args.window_size = model.patch_embed.patch_shape
    if args.finetune:
        utils.finetune(args, model)
    if args.freeze_backbone:
        # linear probing (mem/run_class_finetuning.py:463-471): head / fc_norm train, the trunk runs forward-only.  Applied from
        # args on every start, so a resumed run comes back frozen; nothing about it is stored in the checkpoint.
        frozen = set(model.freeze_backbone())
        for name, _ in model.named_parameters():
            print(f"{'froze' if name in frozen else 'kept'} {name}")
        print("Linear probing: the backbone is frozen (%d tensors), the trunk runs forward-only" % len(frozen))
    model.to(device)
    eng = model.engine                                   # packs parameters into the flat buffers
    # the model's drop-path / dropout generator is seeded from the run seed + rank HERE (every rank its own stream; one state
    # per rank travels with the checkpoints), and the numerics switches of the run are recorded (utils.save_model: "numerics")
    model._dp_stream = utils.DropPathStream()
    model._dp_stream.seed(args.seed + utils.get_rank())
    args.numerics = {"precision": "bf16",
                     "gelu_dg": int(getattr(eng, "epi_gelu", None) == getattr(ops_mod(), "EPI_BIAS_GELU_DG", -1)),
                     "dp_skip": bool(getattr(eng, "dp_skip", False))}
    print("numerics:", args.numerics)
    if args.distributed:
        # BEFORE the EMA twin and the optimizer: both then see the weights rank 0 broadcast.  The loop drives the exchange
        # through model._reducer (engine_for_finetuning.train_one_epoch): update micro-steps only, frozen trunk = head bucket
        exchange = attach_reducer(model, eng, step_exchange=True)
        print("Gradient exchange: %d bucket(s), %d bytes per update step" % (len(exchange.expected), exchange.bytes_per_step))
    model_ema = None
    if args.model_ema:
        model_ema = utils.ModelEma(model, decay=args.model_ema_decay, device="", resume="")
        print("Using EMA with decay = %.8f" % args.model_ema_decay)
    n_parameters = sum(p.numel() for p in model.parameters() if p.requires_grad)
    total_batch_size = args.batch_size * args.update_freq * num_tasks
    steps_per_epoch = max(1, len(data_loader_train) // args.update_freq)
    print("number of params:", n_parameters)
    print("LR = %.8f  Batch size = %d  Update frequency = %d  Training steps per epoch = %d"
          % (args.lr, total_batch_size, args.update_freq, steps_per_epoch))
    num_layers = model.get_num_layers()
    assigner = None
    if args.layer_decay < 1.0:
        assigner = LayerDecayValueAssigner([args.layer_decay ** (num_layers + 1 - i) for i in range(num_layers + 2)])
        print("Assigned values = %s" % str(assigner.values))
    skip = set(model.no_weight_decay())
    if args.disable_weight_decay_on_rel_pos_bias:
        skip |= {"blocks.%d.attn.relative_position_bias_table" % i for i in range(num_layers)}
    optimizer = create_optimizer(args, model, skip_list=skip, get_num_layer=assigner.get_layer_id if assigner else None,
                                 get_layer_scale=assigner.get_scale if assigner else None)
    loss_scaler = utils.NativeScalerWithGradNormCount()
    lr_schedule_values = utils.cosine_scheduler(args.lr, args.min_lr, args.epochs, steps_per_epoch,
                                                warmup_epochs=args.warmup_epochs, warmup_steps=args.warmup_steps)
    if args.weight_decay_end is None:
        args.weight_decay_end = args.weight_decay
    wd_schedule_values = utils.cosine_scheduler(args.weight_decay, args.weight_decay_end, args.epochs, steps_per_epoch)
    criterion = build_criterion(args, mixup_fn)
    print("criterion = %s" % str(criterion))
    utils.auto_load_model(args=args, model=model, model_without_ddp=model, optimizer=optimizer, loss_scaler=loss_scaler,
                          model_ema=model_ema)
    if args.eval:
        test_stats = evaluate(data_loader_val, model, device)
        print(f"Accuracy of the network on the {len(dataset_val)} test images: {test_stats['acc1']:.1f}%")
        if args.output_dir and utils.is_main_process():
            with open(os.path.join(args.output_dir, "eval.txt"), mode="a", encoding="utf-8") as f:
                f.write(json.dumps({f"test_{k}": v for k, v in test_stats.items()}) + "\n")
        utils.cleanup_distributed_mode()
        return test_stats
    print(f"Start training for {args.epochs} epochs")
    start_time = time.time()
    max_accuracy = 0.0
    for epoch in range(args.start_epoch, args.epochs):
        if args.distributed:
            data_loader_train.sampler.set_epoch(epoch)
        train_stats = train_one_epoch(args, model, criterion, data_loader_train, optimizer, device, epoch, loss_scaler,
                                      args.clip_grad, model_ema, mixup_fn, log_writer=None,
                                      start_steps=epoch * steps_per_epoch, lr_schedule_values=lr_schedule_values,
                                      wd_schedule_values=wd_schedule_values, num_training_steps_per_epoch=steps_per_epoch,
                                      update_freq=args.update_freq)
        log_stats = {**{f"train_{k}": v for k, v in train_stats.items()}, "epoch": epoch, "n_parameters": n_parameters}
        if data_loader_val is not None:
            test_stats = evaluate(data_loader_val, model, device)
            print(f"Accuracy of the network on the {len(dataset_val)} test images: {test_stats['acc1']:.1f}%")
            log_stats.update({f"test_{k}": v for k, v in test_stats.items()})
            if model_ema is not None:
                ema_stats = evaluate(data_loader_val, model_ema.ema, device)
                log_stats.update({f"ema_test_{k}": v for k, v in ema_stats.items()})
        # (saved AFTER the evaluation the log line reports, so --eval --resume on the file reproduces that line)
        if args.output_dir and args.save_ckpt:
            if (epoch + 1) % args.save_ckpt_freq == 0 or epoch + 1 == args.epochs:
                utils.save_model(args=args, model=model, model_without_ddp=model, optimizer=optimizer,
                                 loss_scaler=loss_scaler, epoch=epoch, model_ema=model_ema)
            if data_loader_val is not None and max_accuracy < test_stats["acc1"]:
                utils.save_model(args=args, model=model, model_without_ddp=model, optimizer=optimizer,
                                 loss_scaler=loss_scaler, epoch="best", model_ema=model_ema)
        if data_loader_val is not None:
            max_accuracy = max(max_accuracy, test_stats["acc1"])
            print(f"Max accuracy: {max_accuracy:.2f}%")
        if args.output_dir and utils.is_main_process():
            with open(os.path.join(args.output_dir, "log.txt"), mode="a", encoding="utf-8") as f:
                f.write(json.dumps(log_stats) + "\n")
    print("Training time {}".format(str(datetime.timedelta(seconds=int(time.time() - start_time)))))
    utils.cleanup_distributed_mode()


if __name__ == "__main__":
    opts = get_args()
    if opts.output_dir:
        Path(opts.output_dir).mkdir(parents=True, exist_ok=True)
    main(opts)
