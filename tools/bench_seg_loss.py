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

Class weights and OHEM (--what ohem, or both by default): at the same two geometries, per configuration -- class weights
alone; OHEMPixelSampler(thresh=0.7, min_kept=100000); OHEMPixelSampler(thresh=None, min_kept=100000), each sampler with the
class weights, and each on two inputs -- "randn3" (logits randn x 3, keys spread over the range) and "confident" (the label's
class raised by 8 at the nearest low-resolution pixel: most probabilities of the label near 1, as a trained model's; the keys
crowd into a handful of histogram bins, the selection's worst case for LDS atomics) -- two arms:

    hip        SegCrossEntropy(avg_non_ignore=True, class_weight=..., sampler=...): keys + radix select + the weighted kernel
    torch      mem_amd.seg_loss.torch_seg_ce in fp32: F.interpolate + log_softmax + gather, weighted; the sampler as softmax +
               gather + torch.sort + mask

and "plain", the hip loss without either, as the cost to compare with.  One JSON line per geometry and configuration goes to
--out_ohem (default profiles/seg_loss_ohem_ab.jsonl).  A capability, not a race: the figures are reported as found.

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


OHEM_CONFIGS = [("class_weight", None, None), ("ohem_thresh", 0.7, 100000), ("ohem_topk", None, 100000)]


def geometry_ohem(name, B, C, h, w, H, W, a, confident=False):
    """one row per configuration: hip / torch / plain hip, forward + backward, time and peak memory"""
    from mem_amd.seg_loss import OHEMPixelSampler, SegCrossEntropy, torch_seg_ce
    g = torch.Generator(device="cuda").manual_seed(1)
    n = a.sets
    zs, labs = [], []
    for _ in range(n):
        z = torch.randn((B, C, h, w), device="cuda", generator=g) * 3
        if confident:                                   # labels constant over a low-resolution pixel, their class raised by 8
            low = torch.randint(0, C, (B, h, w), device="cuda", generator=g)
            z.scatter_add_(1, low[:, None], torch.full((B, 1, h, w), 8.0, device="cuda"))
            lab = low.repeat_interleave(H // h, 1).repeat_interleave(W // w, 2)
        else:
            lab = torch.randint(0, C, (B, H, W), device="cuda", generator=g)
        lab[torch.rand((B, H, W), device="cuda", generator=g) < 0.2] = 255
        zs.append(z.requires_grad_(True))
        labs.append(lab)
    labs_u8 = [lab.to(torch.uint8) for lab in labs]
    cw = (torch.rand(C, device="cuda", generator=g) * 2 + 0.25).float()
    plain = SegCrossEntropy(avg_non_ignore=True)
    rows = []
    for cfg, T, m in OHEM_CONFIGS:
        smp = None if m is None else OHEMPixelSampler(T, m)
        mod = SegCrossEntropy(avg_non_ignore=True, class_weight=cw, sampler=smp)

        def loss_of(arm, k):
            if arm == "hip":
                return mod(zs[k % n], labs_u8[k % n])
            if arm == "plain":
                return plain(zs[k % n], labs_u8[k % n])
            return torch_seg_ce(zs[k % n], labs[k % n], 255, False, 1.0, True, cw, smp)[0]

        def fwd_bwd(arm):
            def f(k):
                zs[k % n].grad = None
                loss_of(arm, k).backward()
            return f

        arms = ["torch", "plain", "hip"]
        with torch.no_grad():
            l_hip, l_torch = float(loss_of("hip", 0)), float(loss_of("torch", 0))
        n_kept, n_valid = int(mod.last_stats["n_kept"]), int(mod.last_stats["n_valid"])
        # (a pixel whose key sits on the threshold may fall on either side in two fp32 evaluations: the two losses are reported
        # with their relative difference, not asserted equal)
        res = ab({arm: fwd_bwd(arm) for arm in arms}, a.iters, a.reps)
        row = dict(kind="seg_loss_ohem", geometry=name, config=cfg, input="confident" if confident else "randn3",
                   loss_rel_diff=abs(l_hip - l_torch) / max(abs(l_torch), 1e-30), thresh=T, min_kept=m, B=B, C=C, h=h, w=w, H=H, W=W,
                   what="forward_backward", iters=a.iters, reps=a.reps, sets=n, loss_hip=l_hip, loss_torch=l_torch, n_kept=n_kept,
                   n_valid=n_valid, upsampled_mb=round(B * C * H * W * 4 / 1e6, 1), keys_mb=round(B * H * W * 4 / 1e6, 1))
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
        row["hip_over_torch"] = round(row["hip"]["ms"] / row["torch"]["ms"], 4)
        row["hip_over_plain"] = round(row["hip"]["ms"] / row["plain"]["ms"], 4)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "seg_loss_ab.jsonl"))
    ap.add_argument("--out_ohem", default=os.path.join("profiles", "seg_loss_ohem_ab.jsonl"))
    ap.add_argument("--what", default="both", choices=["plain", "ohem", "both"])
    a = ap.parse_args()
    from mem_amd._lib import require_gpu
    require_gpu()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    os.makedirs(os.path.dirname(a.out_ohem) or ".", exist_ok=True)
    for geo in GEOMETRIES:
        jobs = ([(a.out, [geometry(*geo, a)])] if a.what != "ohem" else []) + \
               ([(a.out_ohem, geometry_ohem(*geo, a) + geometry_ohem(*geo, a, confident=True))] if a.what != "plain" else [])
        torch.cuda.empty_cache()
        for out, rows in jobs:
            for row in rows:
                line = json.dumps(row)
                print(line, flush=True)
                with open(out, "a") as f:
                    f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
