"""Evaluate a dVAE tokenizer checkpoint on the HIP path: reconstruction loss, KL to the uniform distribution and codebook
usage on a validation set -- what the reference measures before a pretraining run is spent on a tokenizer
(eventvae/vae/vae_model.py:216-266 `evaluate`, called from eventvae/train_vae.py:380-385).

    python -m mem_amd.eval_tokenizer --expweek 2026-10 --data_path synthetic --input_H 224 --input_W 224 \\
        [--vae_checkpoint vae.pt] [--tokenizer_impl hip|hip_fp16x2|hip_bf16] [--config ncaltech.conf]

takes the flags (and ``--config`` files) of run_mem_pretraining plus ``--vae_checkpoint`` (default:
``--discrete_vae_weight_path``) and prints one JSON line: loss, recon_loss, kl_div, codebook_indices, codebook_usage =
codebook_indices / num_tokens (train_vae.py:385).  There is no torch fallback: the encoder, the decoder and the KL run on
`HipTokenizer` (csrc/conv*.hip, csrc/convt.hip)."""
import json
import sys

import torch

from . import utils


def _images(batch, device):
    """The image batch f32 [B, C, H, W] on the device: a raw event batch (datasets.RawEventDataset.collate: a dict, alone or
    first in a (batch, target) pair) runs its transform chain on the GPU; a tuple batch holds the images first
    (vae_model.py:232)."""
    if isinstance(batch, (tuple, list)) and isinstance(batch[0], dict):
        batch = batch[0]
    if isinstance(batch, dict):
        ev = batch["events"].to(device, non_blocking=True)
        return batch["pipe"](ev, batch["offsets"], batch["draws"])
    return batch[0].to(device, non_blocking=True).float()


@torch.no_grad()
def evaluate(data_loader, tokenizer, device):
    """vae_model.py:216-266 with `tokenizer` a HipTokenizer.  Per batch: ids = get_codebook_indices(images) (the encoder runs
    ONCE: the KL reads the logits that call left in the tokenizer's buffer), recon = decode(ids),
    recon_loss = loss_fn(norm(images), recon), kl_div = sum(kl_uniform_rows(logits)) / batch size (the per-sample mean that
    'batchmean' at :252 names; the reference passes log_uniform of shape [1] as kl_div's input, so torch divides its sum by
    1 there -- its figure is this one times the batch size), loss = recon_loss + kl_div * kl_div_loss_weight.  The averages
    are the reference meter's: it is updated twice per batch, once with n = 1 and once with n = batch size (:257-258), so a
    batch weighs 1 + batch size.  Returns
    {"loss", "recon_loss", "kl_div", "codebook_indices"} (codebook_indices = the number of distinct ids seen)."""
    from . import ops
    vae = tokenizer._model
    meter = utils.MetricLogger(delimiter="  ")
    used = torch.zeros(tokenizer.num_tokens, dtype=torch.bool, device=device)
    for batch in data_loader:
        images = _images(batch, device)
        B = images.shape[0]
        ids = tokenizer.get_codebook_indices(images)
        M = ids.numel()
        kl_div = ops.kl_uniform_rows(tokenizer.logits, M, tokenizer.num_tokens).sum() / B
        used[ids.reshape(-1)] = True
        recon = tokenizer.decode(ids)
        recon_loss = vae.loss_fn(vae.norm(images), recon)
        loss = recon_loss + kl_div * vae.kl_div_loss_weight
        for k, v in (("loss", loss), ("recon_loss", recon_loss), ("kl_div", kl_div)):
            v = v.item()
            meter.update(**{k: v})
            meter.meters[k].update(v, n=B)
    stats = {k: m.global_avg for k, m in meter.meters.items()}
    stats["codebook_indices"] = int(used.sum().item())
    return stats


def main(argv=None):
    import argparse
    from .datasets import build_pretraining_dataset
    from .run_mem_pretraining import get_args
    from .vae_model import DiscreteVAE, HipTokenizer
    argv = list(sys.argv[1:] if argv is None else argv)
    p = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    p.add_argument("--vae_checkpoint", type=str, default=None)
    p.add_argument("--decode_batch", type=int, default=16)
    own, rest = p.parse_known_args(argv)
    args = get_args(rest)
    from ._lib import require_gpu
    require_gpu()
    device = torch.device(args.device)
    torch.manual_seed(args.seed)
    path = own.vae_checkpoint or args.discrete_vae_weight_path
    if path:
        vae = utils.create_d_vae(weight_path=path, d_vae_type=args.discrete_vae_type, device=device,
                                 image_size=(args.input_H2, args.input_W2))
    else:
        print("WARNING: no --vae_checkpoint: evaluating a randomly initialised tokenizer", file=sys.stderr)
        vae = DiscreteVAE(input_H=args.input_H, input_W=args.input_W, num_layers=args.num_layers, num_tokens=args.num_tokens,
                          codebook_dim=32, hidden_dim=64, num_resnet_blocks=0).to(device)
    impl = args.tokenizer_impl if args.tokenizer_impl != "torch" else "hip"
    tokenizer = HipTokenizer(vae.eval(), max_batch=args.batch_size, decode_batch=own.decode_batch,
                             precision={"hip": "fp32", "hip_fp16x2": "fp16x2", "hip_bf16": "bf16"}[impl])
    patch = 2 ** args.num_layers
    args.patch_size = (patch, patch)
    args.window_size = (args.input_H // patch, args.input_W // patch)
    dataset = build_pretraining_dataset(args, is_train=False)
    loader = torch.utils.data.DataLoader(dataset, sampler=torch.utils.data.SequentialSampler(dataset), batch_size=args.batch_size,
                                         num_workers=args.num_workers, pin_memory=args.pin_mem, drop_last=False,
                                         collate_fn=getattr(dataset, "collate", None))
    stats = evaluate(loader, tokenizer, device)
    stats["codebook_usage"] = stats["codebook_indices"] / tokenizer.num_tokens
    print(json.dumps(stats))
    return stats


if __name__ == "__main__":
    main()
