"""The end of a segmentation decode head -- bilinear resize of the logits to the label's size + cross entropy with
ignore_index=255 -- three arms in one process:

    hip        mem_amd.seg_loss.SegCrossEntropy(avg_non_ignore=True): one fused kernel + a finish kernel (csrc/seg_loss.hip),
               backward = one multiply
    torch      F.cross_entropy(F.interpolate(z, size, mode="bilinear"), label, ignore_index=255) in fp32
    autocast   the same under torch.autocast(bfloat16)

at (B = 16, C = 11, 110 x 160 -> 440 x 640) -- the reference's DSEC config -- and (B = 16, C = 19, 128 x 128 -> 512 x 512).
Timed: forward + backward (the gradient with respect to the logits).  Also per arm: the peak of allocated device memory
above what is allocated before the call (inputs excluded), over one forward + backward.

Method of tools/bench_necks.py: the arms alternate inside every repetition, a repetition times `--iters` back-to-back calls
of one arm between two device events, every call takes the next of `--sets` input sets, the figure is the median over
`--reps` repetitions after a warm-up of each arm, with min and max.  The timing is reported, not gated.

Appends one JSON line per geometry to --out (default profiles/seg_loss_ab.jsonl) and prints it.

    python tools/bench_seg_loss.py
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_dense_export import ab  # noqa: E402

GEOMETRIES = [("dsec_b16_c11_110x160", 16, 11, 110, 160, 440, 640), ("b16_c19_128x128", 16, 19, 128, 128, 512, 512)]


def geometry(name, B, C, h, w, H, W, a):
    from mem_amd.seg_loss import SegCrossEntropy
    g = torch.Generator(device="cuda").manual_seed(1)
    n = a.sets
    zs = [(torch.randn((B, C, h, w), device="cuda", generator=g) * 3).requires_grad_(True) for _ in range(n)]
    labs = []
    for _ in range(n):
        lab = torch.randint(0, C, (B, H, W), device="cuda", generator=g)
        lab[torch.rand((B, H, W), device="cuda", generator=g) < 0.2] = 255
        labs.append(lab)
    labs_u8 = [lab.to(torch.uint8) for lab in labs]
    mod = SegCrossEntropy(avg_non_ignore=True)      # F.cross_entropy's mean is over the labels that count: the same number

    def loss_of(arm, k):
        if arm == "hip":
            return mod(zs[k % n], labs_u8[k % n])
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=arm == "autocast"):
            up = F.interpolate(zs[k % n], size=(H, W), mode="bilinear", align_corners=False)
            return F.cross_entropy(up, labs[k % n], ignore_index=255)

    def fwd_bwd(arm):
        def f(k):
            zs[k % n].grad = None
            loss_of(arm, k).backward()
        return f

    arms = ["torch", "autocast", "hip"]
    # the same loss first (fp32 arms), then the clock
    with torch.no_grad():
        l_hip, l_torch = float(loss_of("hip", 0)), float(loss_of("torch", 0))
    assert abs(l_hip - l_torch) <= 1e-5 * abs(l_torch), (l_hip, l_torch)
    res = ab({arm: fwd_bwd(arm) for arm in arms}, a.iters, a.reps)
    row = dict(kind="seg_loss", geometry=name, B=B, C=C, h=h, w=w, H=H, W=W, what="forward_backward", iters=a.iters, reps=a.reps,
               sets=n, loss_hip=l_hip, loss_torch=l_torch, upsampled_mb=round(B * C * H * W * 4 / 1e6, 1))
    for arm, ts in res.items():
        row[arm] = dict(ms=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
    for arm in arms:
        for z in zs:
            z.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fwd_bwd(arm)(0)
        torch.cuda.synchronize()
        row[arm]["peak_mb"] = round((torch.cuda.max_memory_allocated() - before) / 1e6, 1)
    for arm in arms[:-1]:
        row["hip_over_" + arm] = round(row["hip"]["ms"] / row[arm]["ms"], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "seg_loss_ab.jsonl"))
    a = ap.parse_args()
    from mem_amd._lib import require_gpu
    require_gpu()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    for geo in GEOMETRIES:
        row = geometry(*geo, a)
        torch.cuda.empty_cache()
        line = json.dumps(row)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
