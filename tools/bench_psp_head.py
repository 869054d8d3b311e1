"""The PSP decode head (mem_amd.seg_heads.PSPHead, 768 -> 512 -> 11 at pool scales (1, 2, 3, 6): the pyramid branch and the
bottleneck of the reference's UPerHead, with cls_seg) behind a detached input map, forward + backward (gradients to the map and
to all 17 parameters), three arms in one process:

    torch      PSPHead(impl="torch") in fp32 (MIOpen convolutions, torch's pooling, batch norm, interpolate and cat)
    autocast   the same under torch.autocast(bfloat16)
    hip        PSPHead(impl="hip"): the library's bf16 convolution / weight-gradient kernels, csrc/ppm.hip and csrc/seg_head.hip

at B = 16 on 14 x 20 maps (the map UPerHead feeds this branch at the reference's 440 x 640) and on 28 x 40 maps (in_index=2).

Method of tools/bench_fcn_head.py (tools/bench_dense_export.py's): the arms alternate inside every repetition, a repetition
times `--iters` back-to-back calls of one arm between two device events, every call takes the next of `--sets` input sets, the
figure is the median over `--reps` repetitions after a warm-up of each arm, with min and max.  The arms get their own copies of
the head (same values).  Peak memory is torch's max_memory_allocated over one more call of each arm on its own, above what was
allocated before it (the hip arm's per-shape buffers exist by then: `hip_buffers_mib` states them).  The timing is reported,
not gated: the issue sets no target.

`--only hip` runs nothing but that arm's calls, for a kernel trace of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_psp_head.py --only hip --geometry b16_14x20

Appends one JSON line per geometry to --out (default profiles/psp_head_ab.jsonl) and prints it.

    python tools/bench_psp_head.py
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_dense_export import ab  # noqa: E402

GEOMETRIES = [("b16_14x20", 16, 14, 20), ("b16_28x40", 16, 28, 40)]
CIN, C, K, SCALES = 768, 512, 11, (1, 2, 3, 6)
ARMS = ["torch", "autocast", "hip"]


def flops(B, h, w):
    """forward convolution + data gradient + weight gradient of the bottleneck (each 2 R 9 (Cin + n C) C), of the 1x1 branches
    (each 2 B s^2 Cin C) and of the classifier"""
    R = B * h * w
    return 3 * 2.0 * (R * 9 * (CIN + len(SCALES) * C) * C + sum(B * s * s for s in SCALES) * CIN * C + R * C * K)


def arms_of(B, h, w, sets):
    from mem_amd.seg_heads import PSPHead
    torch.manual_seed(0)
    base = PSPHead(in_channels=CIN, channels=C, num_classes=K, in_index=0, pool_scales=SCALES, dropout_ratio=0.1, impl="torch").cuda().train()
    heads = {}
    for arm in ARMS:
        heads[arm] = PSPHead(in_channels=CIN, channels=C, num_classes=K, in_index=0, pool_scales=SCALES, dropout_ratio=0.1,
                             impl="hip" if arm == "hip" else "torch").cuda().train()
        heads[arm].load_state_dict(copy.deepcopy(base.state_dict()), strict=True)
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn((B, CIN, h, w), device="cuda", generator=g).requires_grad_(True) for _ in range(sets)]
    ds = [torch.randn((B, K, h, w), device="cuda", generator=g) for _ in range(sets)]

    def fwd_bwd(arm):
        def f(k):
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=arm == "autocast"):
                out = heads[arm]((xs[k % sets],))
            out.backward(ds[k % sets].to(out.dtype))
        return f

    return heads, fwd_bwd


def geometry(name, B, h, w, a):
    heads, fwd_bwd = arms_of(B, h, w, a.sets)
    res = ab({arm: fwd_bwd(arm) for arm in ARMS}, a.iters, a.reps)
    row = dict(kind="psp_head", geometry=name, B=B, h=h, w=w, Cin=CIN, C=C, K=K, pool_scales=list(SCALES), what="forward_backward",
               iters=a.iters, reps=a.reps, sets=a.sets, gflop=round(flops(B, h, w) / 1e9, 2))
    for arm, ts in res.items():
        row[arm] = dict(ms=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3))
    for arm in ARMS:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fwd_bwd(arm)(0)
        torch.cuda.synchronize()
        row[arm]["peak_mib"] = round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)
    row["hip_buffers_mib"] = round(sum(b.numel() * b.element_size() for b in heads["hip"]._bufs.values()) / 2 ** 20, 1)
    for arm in ARMS[:-1]:
        row["hip_over_" + arm] = round(row["hip"]["ms"] / row[arm]["ms"], 4)
    row["fastest"] = min(ARMS, key=lambda arm: row[arm]["ms"])
    return row


def only(arm, name, B, h, w, a):
    """the calls of one arm and nothing else (a profiler's run): a warm-up, then iters x reps calls"""
    heads, fwd_bwd = arms_of(B, h, w, a.sets)
    step = fwd_bwd(arm)
    for k in range(3):
        step(k)
    torch.cuda.synchronize()
    for k in range(a.iters * a.reps):
        step(k)
    torch.cuda.synchronize()
    print(json.dumps(dict(kind="psp_head_only", arm=arm, geometry=name, calls=a.iters * a.reps, warmup=3)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--geometry", choices=[g[0] for g in GEOMETRIES], default=None)
    ap.add_argument("--only", choices=ARMS, default=None)
    ap.add_argument("--out", default=os.path.join("profiles", "psp_head_ab.jsonl"))
    a = ap.parse_args()
    from mem_amd._lib import require_gpu
    require_gpu()
    geos = [g for g in GEOMETRIES if a.geometry in (None, g[0])]
    if a.only:
        for geo in geos:
            only(a.only, *geo, a)
        return 0
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    for geo in geos:
        row = geometry(*geo, a)
        torch.cuda.empty_cache()
        with open(a.out, "a") as f:
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
