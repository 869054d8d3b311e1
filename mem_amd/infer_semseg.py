"""Stage 4: segmentation inference -- ``python -m mem_amd.infer_semseg --checkpoint iter_N.pth --eval``.

Mirror of mem/semantic_segmentation/tools/test.py (single_gpu_test: predict, evaluate, dump, paint) on the model, data chain and
checkpoints of ``mem_amd.run_semseg``.  ``--test_mode whole|slide`` and ``--flip`` are mmseg 0.30's ``test_cfg.mode`` and the
flip half of ``aug_test``; both end in one ``memhip_seg_predict`` launch per batch (``mem_amd.seg_infer``).

  --eval                       one JSON line: aAcc, mIoU, mAcc, per-class IoU, and the mode, windows and flip used
  --out file.pkl               a pickled list of ``[H, W]`` u8 label arrays in dataset order
  --format-only --imgfile_prefix DIR   class-index PNGs named after the event files
  --show-dir DIR [--opacity, --palette file]   painted PNGs (``seg_infer.paint``; the palette file holds ``r g b`` per line)

Single GPU.  Launchers, distributed runs, ``--gpu-collect`` and ``--aug-test`` parse and are refused by name."""
import argparse
import json
import os
import pickle
from pathlib import Path

import numpy as np
import torch

from . import run_semseg as R
from . import utils

AUG_TEST_WHY = ("--aug-test: --flip is its flip half (both passes' probabilities are averaged); its multi-scale half "
                "(img_ratios 0.5 .. 1.75) is not mirrored: under the reference's own test pipeline (dsec.py:36-44: RandomCrop to "
                "the crop size at test time, zero Pad without un-padding in mmseg 0.30) a ratio != 1 is misaligned with the label "
                "by construction")

# flag -> (the only value taken, why)
REFUSED = {
    "launcher": ("none", "distributed launchers are not carried: single GPU"),
    "distributed": (False, "multi-GPU inference is not set up: single GPU"),
    "world_size": (1, "multi-GPU inference is not set up: single GPU"),
    "gpus": (1, "single GPU"),
    "gpu_collect": (False, "multi-GPU collection of results is not carried: single GPU"),
}


def get_args(argv=None):
    p = argparse.ArgumentParser("mem_amd segmentation inference (stage 4)", allow_abbrev=False)
    R.add_model_data_flags(p)
    p.add_argument("--checkpoint", required=True, help="a checkpoint of mem_amd.run_semseg")
    p.add_argument("--split", default="val")
    p.add_argument("--test_mode", default="whole", choices=["whole", "slide"])
    p.add_argument("--slide_crop", default=None, type=int, nargs=2, metavar=("H", "W"))
    p.add_argument("--slide_stride", default=None, type=int, nargs=2, metavar=("H", "W"))
    p.add_argument("--flip", action="store_true", help="average with the horizontally flipped pass")
    p.add_argument("--max_views_per_call", default=16, type=int, help="samples per model call")
    p.add_argument("--eval", action="store_true")
    p.add_argument("--out", default="")
    p.add_argument("--format-only", "--format_only", dest="format_only", action="store_true")
    p.add_argument("--imgfile_prefix", default="")
    p.add_argument("--show-dir", "--show_dir", dest="show_dir", default="")
    p.add_argument("--opacity", default=0.5, type=float)
    p.add_argument("--palette", default="", help="a text file with 'r g b' per line, one line per class")
    # parsed and refused
    p.add_argument("--aug-test", "--aug_test", dest="aug_test", action="store_true")
    p.add_argument("--launcher", default="none")
    p.add_argument("--distributed", action="store_true")
    p.add_argument("--world_size", default=1, type=int)
    p.add_argument("--gpus", default=1, type=int)
    p.add_argument("--local_rank", default=0, type=int)
    p.add_argument("--gpu-collect", "--gpu_collect", dest="gpu_collect", action="store_true")
    args = p.parse_args(argv)
    if args.aug_test:
        raise NotImplementedError(AUG_TEST_WHY)
    for flag, (only, why) in REFUSED.items():
        if getattr(args, flag) != only:
            raise NotImplementedError(f"--{flag} {getattr(args, flag)}: {why}")
    if args.cat_max_ratio < 1.0:
        raise NotImplementedError(f"--cat_max_ratio {args.cat_max_ratio}: class-balanced crops are not mirrored (dsec.py sets 1.0)")
    if args.test_mode == "slide" and (args.slide_crop is None or args.slide_stride is None):
        raise ValueError("--test_mode slide needs --slide_crop H W and --slide_stride H W")
    if args.test_mode == "whole" and (args.slide_crop is not None or args.slide_stride is not None):
        raise ValueError("--slide_crop / --slide_stride go with --test_mode slide")
    if not (args.eval or args.out or args.format_only or args.show_dir):
        raise ValueError("nothing to do: give at least one of --eval, --out, --format-only, --show-dir")
    if args.eval and args.format_only:
        raise ValueError("--eval and --format-only cannot both be given")
    if args.out and not args.out.endswith((".pkl", ".pickle")):
        raise ValueError(f"--out {args.out}: the output file must be a .pkl / .pickle file")
    if args.format_only and not args.imgfile_prefix:
        raise ValueError("--format-only needs --imgfile_prefix DIR")
    if not 0.0 < args.opacity <= 1.0:
        raise ValueError(f"--opacity {args.opacity}: in (0, 1]")
    args.val_split = args.split
    return R.resolve_model_args(args)


def load_palette(path, num_classes):
    """u8 ``[num_classes, 3]`` from a text file with ``r g b`` per line."""
    rows = [[int(v) for v in line.split()] for line in open(path) if line.strip()]
    if len(rows) < num_classes or any(len(r) != 3 or min(r) < 0 or max(r) > 255 for r in rows):
        raise ValueError(f"--palette {path}: {num_classes} lines of 'r g b' with values 0..255 are expected")
    return torch.tensor(rows[:num_classes], dtype=torch.uint8)


def sample_names(dataset):
    """The output file stem of every sample: the event file's path below ``imgs/<split>`` without its suffix."""
    if dataset.synthetic:
        return ["synthetic_%06d" % i for i in range(len(dataset))]
    img_dir = os.path.join(dataset.root, "imgs", dataset.split)
    return [os.path.relpath(ev, img_dir)[:-len(".npy")] for ev, _ in dataset.pairs]


def _save_png(array, folder, stem):
    from PIL import Image
    path = Path(folder) / (stem + ".png")
    path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(array).save(path)
    return str(path)


def build_inferencer(args):
    """-> (``SegInferencer`` on the checkpoint's model in eval mode, the dataset of ``--split``, the checkpoint's iteration)"""
    from .seg_infer import SegInferencer
    device = torch.device(args.device)
    cfg, pipeline = R.build_pipeline(args)
    model = R.build_model(args)
    model.to(device)
    model.backbone.engine                                 # packs the backbone's parameters into the flat buffers
    dataset = R.build_dataset(args, cfg, train=False)
    if len(dataset.CLASSES) != args.num_classes:
        raise ValueError(f"labels.txt names {len(dataset.CLASSES)} classes, --num_classes is {args.num_classes}")
    it = R.load_checkpoint(args.checkpoint, model)
    model.eval()
    inf = SegInferencer(model, pipeline, mode=args.test_mode, crop_size=args.slide_crop, stride=args.slide_stride, flip=args.flip,
                        max_views_per_call=args.max_views_per_call)
    return inf, dataset, it


def main(args):
    """Returns the record it prints as one JSON line: the mode, windows and flip used, the number of samples, the metrics
    under ``--eval`` and the files written."""
    from ._lib import require_gpu
    from .seg_infer import default_palette, paint
    require_gpu()
    utils.cap_host_threads(4)
    torch.manual_seed(args.seed)
    device = torch.device(args.device)
    inf, dataset, it = build_inferencer(args)
    names = sample_names(dataset)
    palette = (load_palette(args.palette, args.num_classes) if args.palette else default_palette(args.num_classes)).to(device)
    results, written = [], {"format": [], "show": []}
    keep = bool(args.out)

    def on_batch(indices, pred):
        host = pred.cpu().numpy()
        if keep:
            results.extend(np.array(host[k]) for k in range(len(indices)))
        if args.format_only:
            written["format"] += [_save_png(host[k], args.imgfile_prefix, names[i]) for k, i in enumerate(indices)]
        if args.show_dir:
            shown = paint(pred, inf.image_u8(), palette, args.opacity).cpu().numpy()
            written["show"] += [_save_png(shown[k], args.show_dir, names[i]) for k, i in enumerate(indices)]

    metrics = inf.evaluate(dataset, args.samples_per_gpu, args.workers_per_gpu, on_batch)
    rec = {"iter": it, **inf.describe(), "samples": len(dataset)}
    if args.eval:
        rec.update(metrics)
    if args.out:
        with open(args.out, "wb") as f:
            pickle.dump(results, f)
        rec["out"] = args.out
    if args.format_only:
        rec["formatted"] = len(written["format"])
    if args.show_dir:
        rec["shown"] = len(written["show"])
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    main(get_args())
