"""A/B of the segmentation data chain at the reference's shape: B = 16 samples, 440 x 640 canvas, ratio 1.0 .. 1.01, crop
440 x 640, net 512 x 512 (mem_amd.seg_data.SegBatchPipeline) against the same chain written with torch ops on the device, one
sample at a time as the reference's transforms are (the sizes differ per sample).  Both arms start from the same events on the
host and end with (img f32 [B, 3, 512, 512], label u8 [B, 440, 640]) on the device; RandAugment is the library's kernel in both.
The arms alternate inside one process; a figure is the median over the repetitions of the wall time between two device
synchronisations (the chain's host work -- packing, uploads, launches -- is part of what a training step waits for).

    python tools/bench_seg_data.py [--batch 16] [--events 180000] [--reps 15] [--out profiles/semseg_ab.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_chain(cfg, events, offsets_h, labels, draws, train):
    from mem_amd._lib import C, check, lib, stream_ptr
    from mem_amd.augment import RANDAUG_DTYPE, randaug_record
    from mem_amd.seg_data import randaug_of
    dev = labels.device
    H, W = cfg.canvas
    ch, cw = cfg.crop_size
    B = len(draws)
    out = torch.empty((B, 3) + cfg.net_size, device=dev)
    lab_out = torch.empty((B, ch, cw), dtype=torch.uint8, device=dev)
    if train:
        recs = np.zeros((B, 2), dtype=RANDAUG_DTYPE)
        for b in range(B):
            for k in range(2):
                recs[b, k] = randaug_record(*randaug_of(cfg, draws[b]["ra"][k]))
        recs_d = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to(dev)
    for b in range(B):
        ev = events[offsets_h[b]:offsets_h[b + 1]]
        idx = ev[:, 0].long() + W * ev[:, 1].long()
        pos = torch.bincount(idx[ev[:, 3] == 1], minlength=H * W)
        neg = torch.bincount(idx[ev[:, 3] == -1], minlength=H * W)
        img = torch.stack([pos, torch.zeros_like(pos), neg]).view(3, H, W).to(torch.uint8)      # wraps at 256
        h, w = cfg.dims_of(float(draws[b]["ratio"]))
        x = F.interpolate(img[None].float(), size=(h, w), mode="bilinear", align_corners=False)[0]
        x = torch.floor(x + 0.5)                                                                  # the 8-bit resize
        v = x[0::2]
        thr = v.mean() + cfg.num_stds * v.std()
        hot = torch.maximum(x[0], x[2]) > thr
        x[0::2] = torch.where(hot[None], torch.zeros_like(v), v)
        m = x.max()
        x = x / torch.where(m == 0, torch.ones_like(m), m) * 255.
        if train:
            a = x.to(torch.uint8).contiguous()
            for k in range(2):
                o = torch.empty_like(a)
                check(lib.memhip_rand_augment_u8(C.c_void_p(a.data_ptr()), C.c_void_p(o.data_ptr()),
                                                 C.c_void_p(recs_d.data_ptr() + (2 * b + k) * RANDAUG_DTYPE.itemsize), 1, h, w,
                                                 stream_ptr()), "rand_augment")
                a = o
            x = a.float()
        top, left, flip = int(draws[b]["top"]), int(draws[b]["left"]), int(draws[b]["flip"])
        lab = F.interpolate(labels[b][None, None].float(), size=(h, w), mode="nearest")[0, 0].to(torch.uint8)
        x, lab = x[:, top:top + ch, left:left + cw], lab[top:top + ch, left:left + cw]
        if flip:
            x, lab = x.flip(2), lab.flip(1)
        x = F.pad(x[[2, 1, 0]], (0, cw - x.shape[2], 0, ch - x.shape[1]))
        lab_out[b] = F.pad(lab, (0, cw - lab.shape[1], 0, ch - lab.shape[0]), value=255)
        out[b] = F.interpolate(x[None], size=cfg.net_size, mode="bilinear", align_corners=False)[0]
    return out, lab_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--events", type=int, default=180000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from mem_amd.seg_data import EventSegDataset, SegBatchPipeline, SegPipelineConfig
    cfg = SegPipelineConfig()
    pipe = SegBatchPipeline(cfg)
    results = []
    for train in (True, False):
        ds = EventSegDataset("synthetic", "train", cfg, train=train, n_synthetic=a.batch, synthetic_events=a.events)
        events, offsets, labels, draws = ds.collate([ds[(i, 0)] for i in range(a.batch)])
        events, labels = events.pin_memory(), labels.pin_memory()
        off_h = offsets.tolist()

        def hip():
            return pipe(events, offsets, labels, draws, train)

        def torch_arm():
            return torch_chain(cfg, events.cuda(non_blocking=True), off_h, labels.cuda(non_blocking=True), draws, train)
        times = {"hip": [], "torch": []}
        for r in range(a.warmup + a.reps):
            for name, fn in (("hip", hip), ("torch", torch_arm)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r >= a.warmup:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        io, lo = hip()
        it, lt = torch_arm()
        rec = {"bench": "seg_data", "mode": "train" if train else "test", "batch": a.batch, "events_per_sample": int(off_h[1]),
               "canvas": list(cfg.canvas), "net_size": list(cfg.net_size), "reps": a.reps,
               "hip_ms": round(statistics.median(times["hip"]), 3), "torch_ms": round(statistics.median(times["torch"]), 3),
               "hip_ms_min": round(min(times["hip"]), 3), "torch_ms_min": round(min(times["torch"]), 3),
               "label_mismatch_px": int((lo != lt).sum()), "img_max_abs_diff": round(float((io - it).abs().max()), 4),
               "img_mean_abs_diff": round(float((io - it).abs().mean()), 6), "device": torch.cuda.get_device_name(0)}
        rec["speedup"] = round(rec["torch_ms"] / rec["hip_ms"], 2)
        print(json.dumps(rec), flush=True)
        results.append(rec)
    if a.out:
        with open(a.out, "a") as f:
            for rec in results:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
