"""Stage 1 of the pipeline: train the event dVAE tokenizer on the HIP path (reference entrypoint: eventvae/train_vae.py).

    python -m mem_amd.train_vae --data_path synthetic --output_dir runs/vae --input_H 224 --input_W 224 --num_layers 4 \\
        --num_tokens 8192 --emb_dim 512 --hidden_dim 384 --num_resnet_blocks 3 --batch_size 32 --epochs 20

takes the flags of train_vae.py:43-125 under the same names and aliases, with the same defaults, `--config FILE` included
(flat `key = value` lines, read like run_mem_pretraining reads them; flags on the command line win).  The model runs on
`vae_train.DVAEEngine` (explicit forward / backward on the hand-written kernels, Adam with the clip folded in); there is no
torch fallback.  The loop is train_vae.py:304-396 as written, quirks included: the temperature and the ExponentialLR advance only
when `i % 10000 == 0` (i restarts with every epoch), with exp(-anneal_rate * global_step); `evaluate` runs every 25th epoch
(mem_amd.eval_tokenizer.evaluate on a HipTokenizer of the live weights); checkpoint-{epoch}.pt / checkpoint-final.pt hold
{'hparams', 'epoch', 'optimizer', 'args', 'weights'} -- utils.create_d_vae loads them, and 'optimizer' is a torch.optim.Adam
state dict.

Single GPU only: WORLD_SIZE > 1 is refused, and so are the reference's distributed-backend and DeepSpeed flags, by name.
Weights & Biases logging is not provided: --disable_wandb parses and changes nothing; one JSON line per logged step goes to
stdout instead.

--kl_loss_weight: the weight of kl_div = sum over the token rows / batch size, the project's one definition
(eval_tokenizer.evaluate).  The reference's F.kl_div(..., 'batchmean') divides by 1 there, so its kl_div -- and the effect of
the same weight -- is batch_size times larger: multiply a reference run's weight by its batch size to reproduce it here."""
import argparse
import json
import math
import os
import sys

import torch

REFUSED = {
    "distributed_backend": "--distributed_backend / --distr_backend: dVAE training here is single-GPU, there is no Horovod or DeepSpeed backend",
    "deepspeed": "--deepspeed: dVAE training here is single-GPU, there is no DeepSpeed backend",
}


def get_args(argv=None):
    p = argparse.ArgumentParser("dVAE training script", allow_abbrev=False,
                                epilog="--config FILE: a file of `key = value` lines read as flags; flags on the command line win")
    p.add_argument("--data_path", type=str, required=True, help="dataset folder (train/ and val/ of .npy event files), or 'synthetic'")
    p.add_argument("--output_dir", default="runs/vae", type=str)
    p.add_argument("--expweek", default="09-05", type=str)
    p.add_argument("--expname", default="test", type=str)
    p.add_argument("--eval_data_path", default=None, type=str)
    p.add_argument("--imagenet_default_mean_and_std", default=False, action="store_true")
    p.add_argument("--data_set", default="npy", choices=["CIFAR", "IMNET", "image_folder", "npy", "dsec_semseg"], type=str)
    p.add_argument("--timesurface", type=int, default=0)
    p.add_argument("--hotpix_num_stds", type=float, default=10)
    p.add_argument("--hotpixfilter", type=int, default=1)
    p.add_argument("--logtrafo", type=int, default=0)
    p.add_argument("--gammatrafo", type=int, default=0)
    p.add_argument("--gamma", type=float, default=0.5)
    p.add_argument("--normalize_events", type=int, default=1)
    p.add_argument("--slice_max_evs", type=int, default=30000)
    p.add_argument("--max_random_shift_evs", type=int, default=15)
    p.add_argument("--rand_aug", type=int, default=1)
    p.add_argument("--disable_eval", action="store_true", default=False)
    p.add_argument("--dist_eval", action="store_true", default=False)
    p.add_argument("--input_size", default=224, type=int)
    p.add_argument("--color_jitter", type=float, default=0.0, metavar="PCT")
    p.add_argument("--aa", type=str, default="rand-m9-mstd0.5-inc1", metavar="NAME")
    p.add_argument("--smoothing", type=float, default=0.1)
    p.add_argument("--train-interpolation", type=str, default="bicubic")
    p.add_argument("--reprob", type=float, default=0.25, metavar="PCT")
    p.add_argument("--remode", type=str, default="pixel")
    p.add_argument("--recount", type=int, default=1)
    p.add_argument("--resplit", action="store_true", default=False)
    p.add_argument("--input_H", type=int, default=128)
    p.add_argument("--input_W", type=int, default=128)
    p.add_argument("--weights", type=str, default=None, help="checkpoint to start from ({'hparams', 'weights', ...})")
    p.add_argument("--num_workers", default=4, type=int)
    p.add_argument("--pin_mem", action="store_true")
    p.add_argument("--save_ckpt_freq", "--vae_save_ckpt_freq", default=5, type=int)
    p.add_argument("--resize", action="store_true", default=False)
    p.add_argument("--disable_wandb", action="store_true", default=False, help="parses; there is no Weights & Biases logging here")
    # the reference's distributed_utils.wrap_arg_parser: parsed, refused by name
    p.add_argument("--distributed_backend", "--distr_backend", type=str, default=None, help="refused: single GPU only")
    p.add_argument("--deepspeed", nargs="?", const=True, default=None, help="refused: single GPU only")
    p.add_argument("--local_rank", type=int, default=-1)
    t = p.add_argument_group("Training settings")
    t.add_argument("--epochs", "--vae_epochs", type=int, default=20)
    t.add_argument("--start_epoch", default=0, type=int, metavar="N")
    t.add_argument("--batch_size", "--vae_batch_size", type=int, default=8)
    t.add_argument("--lr", "--vae_lr", type=float, default=1e-3)
    t.add_argument("--lr_decay_rate", "--vae_lr_decay", type=float, default=0.98)
    t.add_argument("--starting_temp", type=float, default=1.0)
    t.add_argument("--temp_min", type=float, default=0.5)
    t.add_argument("--anneal_rate", type=float, default=1e-6)
    t.add_argument("--num_images_save", type=int, default=4)
    m = p.add_argument_group("Model settings")
    m.add_argument("--num_tokens", type=int, default=8192)
    m.add_argument("--num_layers", type=int, default=3)
    m.add_argument("--num_resnet_blocks", "--vae_num_resnet_blocks", type=int, default=2)
    m.add_argument("--loss", "--vae_loss", type=str, default="mse", choices=["mse", "smooth_l1", "cosine"])
    m.add_argument("--emb_dim", type=int, default=512)
    m.add_argument("--hidden_dim", "--vae_hidden_dim", type=int, default=256)
    m.add_argument("--kl_loss_weight", "--vae_kl_loss_weight", type=float, default=0.0,
                   help="weight of kl_div = sum over the token rows / batch size (the project's definition; the reference's "
                        "'batchmean' figure is batch_size times this one, so the same weight acts batch_size times weaker here)")
    m.add_argument("--clip", "--vae_grad_clip", type=float, default=1e-3)
    m.add_argument("--straight_through", "--vae_straight_through", type=int, default=0)
    # not the reference's: the device, the seed, a step limit for smoke runs, the size of the synthetic stand-in
    p.add_argument("--device", default="cuda")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--max_steps", default=0, type=int, help="stop after this many steps in total (0: no limit)")
    p.add_argument("--synthetic_samples", default=64, type=int)
    from .run_mem_pretraining import _config_file_args
    # --config FILE (the reference's configargparse file, train_vae.py:43-47): flat `key = value` lines become flags placed
    # in front of the command line, so explicit flags win; the vae_* aliases above are the keys of the pipeline's shared file
    return p.parse_known_args(_config_file_args(list(sys.argv[1:] if argv is None else argv)))[0]


def refuse(args, environ=None):
    """What this entrypoint does not provide, by name."""
    environ = os.environ if environ is None else environ
    for name, why in REFUSED.items():
        if getattr(args, name) is not None:
            raise SystemExit("refused " + why)
    if int(environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("refused WORLD_SIZE=%s: mem_amd.train_vae is single-GPU only (no data-parallel dVAE training)" % environ["WORLD_SIZE"])


class Schedule:
    """The temperature and learning rate of train_vae.py:342-353: both advance only when i % 10000 == 0 (i = the iteration
    inside the epoch), the temperature by exp(-anneal_rate * global_step) down to temp_min, the rate by ExponentialLR's
    lr *= gamma."""

    def __init__(self, args):
        self.temp, self.lr, self.global_step = args.starting_temp, args.lr, 0
        self.anneal_rate, self.temp_min, self.gamma = args.anneal_rate, args.temp_min, args.lr_decay_rate

    def after_step(self, i):
        if i % 10000 == 0:
            self.temp = max(self.temp * math.exp(-self.anneal_rate * self.global_step), self.temp_min)
            self.lr = self.lr * self.gamma
        self.global_step += 1


def _pretraining_args(args, data_path):
    """The namespace datasets.build_pretraining_dataset reads, from this script's flags."""
    from .run_mem_pretraining import get_args as pt_args
    a = pt_args(["--expweek", args.expweek, "--data_path", data_path, "--input_H", str(args.input_H), "--input_W", str(args.input_W),
                 "--batch_size", str(args.batch_size), "--num_layers", str(args.num_layers), "--num_tokens", str(args.num_tokens),
                 "--synthetic_samples", str(args.synthetic_samples), "--num_workers", str(args.num_workers)])
    for k in ("timesurface", "hotpix_num_stds", "hotpixfilter", "logtrafo", "gammatrafo", "gamma", "normalize_events", "slice_max_evs",
              "max_random_shift_evs", "rand_aug", "data_set", "imagenet_default_mean_and_std", "resize"):
        setattr(a, k, getattr(args, k))
    patch = 2 ** args.num_layers
    a.patch_size = (patch, patch)
    a.window_size = (args.input_H // patch, args.input_W // patch)
    return a


def _loader(args, data_path, is_train):
    from .datasets import build_pretraining_dataset
    ds = build_pretraining_dataset(_pretraining_args(args, data_path), is_train=is_train)
    sampler = torch.utils.data.RandomSampler(ds) if is_train else torch.utils.data.SequentialSampler(ds)
    return torch.utils.data.DataLoader(ds, sampler=sampler, batch_size=args.batch_size, num_workers=args.num_workers, pin_memory=args.pin_mem,
                                       drop_last=is_train, collate_fn=getattr(ds, "collate", None))


def main(argv=None):
    from . import utils
    from ._lib import require_gpu
    from .eval_tokenizer import _images, evaluate
    from .vae_model import DiscreteVAE, HipTokenizer
    from .vae_train import DVAEEngine
    args = get_args(argv)
    refuse(args)
    require_gpu()
    print("no Weights & Biases logging here (with or without --disable_wandb): one JSON line per logged step goes to stdout", flush=True)
    device = torch.device(args.device)
    torch.manual_seed(args.seed)
    import numpy as np
    np.random.seed(args.seed)
    loader = _loader(args, args.data_path, True)
    loader_val = None if args.disable_eval else _loader(args, args.eval_data_path or args.data_path, False)
    assert len(loader.dataset) > 0, "folder does not contain any images"
    print(f"{len(loader.dataset)} samples found for training")
    hparams, weights, opt_state = None, None, None
    if args.weights:
        ck = torch.load(args.weights, map_location="cpu", weights_only=False)
        hparams, weights, opt_state = ck["hparams"], ck["weights"], ck.get("optimizer")
        args.start_epoch = ck.get("epoch", -1) + 1
    if hparams is None:
        hparams = dict(input_H=args.input_H, input_W=args.input_W, num_layers=args.num_layers, num_tokens=args.num_tokens,
                       codebook_dim=args.emb_dim, hidden_dim=args.hidden_dim, num_resnet_blocks=args.num_resnet_blocks)
        channels = _images(next(iter(loader)), device).shape[1]
        if channels != 3:                                    # the reference's module default
            hparams["channels"] = channels
    vae = DiscreteVAE(**hparams, loss=args.loss, kl_div_loss_weight=args.kl_loss_weight, straight_through=bool(args.straight_through))
    if weights is not None:
        print("Loading checkpoint from epoch %d" % (args.start_epoch - 1))
        vae.load_state_dict(weights)
    vae = vae.to(device).train()
    engine = DVAEEngine(vae, seed=args.seed)
    if opt_state is not None:
        engine.load_optimizer_state_dict(opt_state)
    print("Number of parameters in vae:", sum(p.numel() for p in vae.parameters()))
    sched = Schedule(args)

    def save_model(path, epoch):
        print(f"Saving model to {path}")
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        torch.save({"hparams": hparams, "epoch": epoch, "optimizer": engine.optimizer_state_dict(sched.lr), "args": args,
                    "weights": {k: v.detach().cpu().clone() for k, v in vae.state_dict().items()}}, path)

    print(f"Start training for {args.epochs} epochs, start epoch {args.start_epoch}, batch size {args.batch_size}")
    done = False
    for epoch in range(args.start_epoch, args.epochs):
        meter = utils.MetricLogger(delimiter="  ")
        for i, batch in enumerate(loader):
            images = _images(batch, device)
            loss, recon_loss, kl_div = engine.forward_backward(images, sched.temp)
            engine.step(sched.lr, max_norm=args.clip if args.clip > 0 else 0.0)
            sched.after_step(i)
            if i % 10 == 0 or args.max_steps:
                v = float(loss)
                meter.update(loss=v)
                print(json.dumps({"epoch": epoch, "iter": i, "step": sched.global_step, "loss": v, "recon_loss": float(recon_loss),
                                  "kl_div": float(kl_div), "lr": sched.lr, "temp": sched.temp}), flush=True)
            if args.max_steps and sched.global_step >= args.max_steps:
                done = True
                break
        if (epoch + 1) % 25 == 0 and loader_val is not None:
            tok = HipTokenizer(vae.eval(), max_batch=args.batch_size, precision="bf16")
            stats = evaluate(loader_val, tok, device)
            vae.train()
            print(json.dumps({"epoch": epoch, "test_loss": stats["loss"], "codebook_usage": stats["codebook_indices"] / args.num_tokens}), flush=True)
        if (epoch + 1) % args.save_ckpt_freq == 0 or epoch + 1 == args.epochs:
            save_model(os.path.join(args.output_dir, f"checkpoint-{epoch}.pt"), epoch)
        if done:
            break
    save_model(os.path.join(args.output_dir, "checkpoint-final.pt"), args.epochs - 1)


if __name__ == "__main__":
    main()
