"""The feature-pyramid necks fpn1 + fpn2 of the segmentation backbone, three arms in one process:

    torch      today's path: the nn.ConvTranspose2d / nn.SyncBatchNorm / nn.GELU modules in fp32 (MIOpen)
    autocast   the same modules under torch.autocast(bfloat16)
    fused      mem_amd.necks.FusedNecks: bf16 GEMMs of this library + the kernels of csrc/necks.hip

at (B = 256, 14 x 14, D = 768) -- the 224^2 finetuning batch -- and (B = 16, 32 x 32, D = 768) -- the 512^2 crop of the
reference's segmentation config.  Timed: the forward alone (train(), no_grad: batch statistics, nothing kept) and forward +
backward (gradients to the map and to all eight parameters) of both necks together.

Method of tools/bench_dense_export.py: the arms alternate inside every repetition, a repetition times `--iters` back-to-back
calls of one arm between two device events, every call takes the next of `--sets` input sets (map and output gradients), the
figure is the median over `--reps` repetitions after a warm-up of each arm, with min and max.  The arms get their own copies
of the modules (same values).  The timing is reported, not gated.

Appends one JSON line per geometry and pass to --out (default profiles/necks_ab.jsonl) and prints it.

    python tools/bench_necks.py
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_dense_export import ab  # noqa: E402

GEOMETRIES = [("b256_14x14", 256, 14, 14, 768), ("b16_32x32", 16, 32, 32, 768)]


def flops_forward(B, Hp, Wp, D):
    """The three transposed convolutions: [R, D] x [D, 4D] at R, 4R (fpn1) and R (fpn2) pixel rows."""
    return 2.0 * (6 * B * Hp * Wp) * D * 4 * D


def modules(D):
    torch.manual_seed(0)
    fpn1 = nn.Sequential(nn.ConvTranspose2d(D, D, 2, 2), nn.SyncBatchNorm(D), nn.GELU(), nn.ConvTranspose2d(D, D, 2, 2))
    fpn2 = nn.Sequential(nn.ConvTranspose2d(D, D, 2, 2))
    for c in (fpn1[0], fpn1[3], fpn2[0]):
        nn.init.trunc_normal_(c.weight, std=0.02)
    return nn.ModuleList([fpn1, fpn2]).cuda().train()


def geometry(name, B, Hp, Wp, D, a):
    from mem_amd.necks import FusedNecks
    base = modules(D)
    mods = {arm: copy.deepcopy(base) for arm in ("torch", "autocast", "fused")}
    fused = FusedNecks(mods["fused"][0], mods["fused"][1])
    g = torch.Generator(device="cuda").manual_seed(1)
    n = a.sets
    xs = [torch.randn((B, D, Hp, Wp), device="cuda", generator=g).requires_grad_(True) for _ in range(n)]
    d1 = [torch.randn((B, D, 4 * Hp, 4 * Wp), device="cuda", generator=g) for _ in range(n)]
    d2 = [torch.randn((B, D, 2 * Hp, 2 * Wp), device="cuda", generator=g) for _ in range(n)]

    def call(arm, x):
        if arm == "fused":
            return fused.fpn1_apply(x), fused.fpn2_apply(x)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=arm == "autocast"):
            return mods[arm][0](x), mods[arm][1](x)

    def fwd(arm):
        def f(k):
            with torch.no_grad():
                call(arm, xs[k % n])
        return f

    def fwd_bwd(arm):
        def f(k):
            o1, o2 = call(arm, xs[k % n])
            torch.autograd.backward([o1, o2], [d1[k % n].to(o1.dtype), d2[k % n].to(o2.dtype)])
        return f

    arms = ["torch", "autocast", "fused"]
    try:
        fwd("autocast")(0)
        torch.cuda.synchronize()
    except RuntimeError as e:
        print("autocast arm not available at %s: %s" % (name, str(e).splitlines()[0]))
        arms.remove("autocast")
    rows = []
    for what, make in (("forward", fwd), ("forward_backward", fwd_bwd)):
        res = ab({arm: make(arm) for arm in arms}, a.iters, a.reps)
        row = dict(kind="necks", geometry=name, B=B, Hp=Hp, Wp=Wp, D=D, what=what, iters=a.iters, reps=a.reps, sets=n,
                   gflop_forward=round(flops_forward(B, Hp, Wp, D) / 1e9, 2))
        for arm, ts in res.items():
            row[arm] = dict(ms=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3))
        for arm in arms[:-1]:
            row["fused_over_" + arm] = round(row["fused"]["ms"] / row[arm]["ms"], 4)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "necks_ab.jsonl"))
    a = ap.parse_args()
    from mem_amd._lib import require_gpu
    require_gpu()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    for geo in GEOMETRIES:
        rows = geometry(*geo, a)
        torch.cuda.empty_cache()
        with open(a.out, "a") as f:
            for r in rows:
                line = json.dumps(r)
                print(line, flush=True)
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
