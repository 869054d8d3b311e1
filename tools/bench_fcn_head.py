"""The FCN decode head (mem_amd.seg_heads.FCNHead, 768 -> 256 -> 11, the reference's auxiliary head) behind a detached input
map, forward + backward (gradients to the map and to all five parameters), three arms in one process:

    torch      FCNHead(impl="torch") in fp32 (MIOpen convolutions, torch's batch norm)
    autocast   the same under torch.autocast(bfloat16)
    hip        FCNHead(impl="hip"): the library's bf16 convolution / weight-gradient kernels + csrc/seg_head.hip

at B = 16 on 32 x 32 maps (the 512^2 crop of the reference's segmentation config) and on 28 x 40 maps.

Method of tools/bench_dense_export.py: the arms alternate inside every repetition, a repetition times `--iters` back-to-back
calls of one arm between two device events, every call takes the next of `--sets` input sets (map and logit gradients), the
figure is the median over `--reps` repetitions after a warm-up of each arm, with min and max.  The arms get their own copies
of the head (same values).  Peak memory is torch's max_memory_allocated over one more call of each arm on its own, above what
was allocated before it.  The split of the hip arm over its kernels comes from a separate pass with a device-event pair around
every library call of the walk (the events add launch gaps: the split's sum is above the arm's figure).  The timing is
reported, not gated: the issue sets no target.

Appends one JSON line per geometry to --out (default profiles/fcn_head_ab.jsonl) and prints it.

    python tools/bench_fcn_head.py
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

GEOMETRIES = [("b16_32x32", 16, 32, 32), ("b16_28x40", 16, 28, 40)]
CIN, C, K = 768, 256, 11
WALK = ("map_to_nhwc_pad", "conv2d_nhwc", "bn_stats_nhwc", "bnhead_fwd", "bnhead_bwd_sums", "bnhead_bwd_apply", "conv_wgrad",
        "nhwc_pad_to_map")


def flops(B, h, w):
    """forward convolution + data gradient + weight gradient (each 2 R 9 Cin C) and the classifier three times"""
    R = B * h * w
    return 3 * 2.0 * R * 9 * CIN * C + 3 * 2.0 * R * C * K


def split(head, step, iters):
    """device time per library call of the hip walk, ms per forward + backward; conv2d_nhwc is split into forward and dgrad"""
    from mem_amd import ops
    real = {n: getattr(ops, n) for n in WALK}
    marks = []

    def wrap(name):
        def f(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = real[name](*args, **kw)
            e1.record()
            key = name
            if name == "conv2d_nhwc":
                key = "conv2d_nhwc.forward" if args[0].shape[-1] == CIN else "conv2d_nhwc.dgrad"
            marks.append((key, e0, e1))
            return r
        return f

    try:
        for n in WALK:
            setattr(ops, n, wrap(n))
        for k in range(iters):
            step(k)
        torch.cuda.synchronize()
    finally:
        for n in WALK:
            setattr(ops, n, real[n])
    out = {}
    for key, e0, e1 in marks:
        out[key] = out.get(key, 0.0) + e0.elapsed_time(e1) / iters
    return {k: round(v, 4) for k, v in out.items()}


def geometry(name, B, h, w, a):
    from mem_amd.seg_heads import FCNHead
    torch.manual_seed(0)
    base = FCNHead(in_channels=CIN, channels=C, num_classes=K, in_index=0, dropout_ratio=0.1, impl="torch").cuda().train()
    heads = {arm: copy.deepcopy(base) for arm in ("torch", "autocast", "hip")}
    heads["hip"].impl = "hip"
    g = torch.Generator(device="cuda").manual_seed(1)
    n = a.sets
    xs = [torch.randn((B, CIN, h, w), device="cuda", generator=g).requires_grad_(True) for _ in range(n)]
    ds = [torch.randn((B, K, h, w), device="cuda", generator=g) for _ in range(n)]

    def fwd_bwd(arm):
        def f(k):
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=arm == "autocast"):
                out = heads[arm]((xs[k % n],))
            out.backward(ds[k % n].to(out.dtype))
        return f

    arms = ["torch", "autocast", "hip"]
    res = ab({arm: fwd_bwd(arm) for arm in arms}, a.iters, a.reps)
    row = dict(kind="fcn_head", geometry=name, B=B, h=h, w=w, Cin=CIN, C=C, K=K, what="forward_backward", iters=a.iters, reps=a.reps,
               sets=n, gflop=round(flops(B, h, w) / 1e9, 2))
    for arm, ts in res.items():
        row[arm] = dict(ms=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3))
    for arm in arms:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fwd_bwd(arm)(0)
        torch.cuda.synchronize()
        row[arm]["peak_mib"] = round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)
    row["hip_buffers_mib"] = round(sum(b.numel() * b.element_size() for b in heads["hip"]._bufs.values()) / 2 ** 20, 1)
    for arm in arms[:-1]:
        row["hip_over_" + arm] = round(row["hip"]["ms"] / row[arm]["ms"], 4)
    row["fastest"] = min(arms, key=lambda arm: row[arm]["ms"])
    row["hip_split_ms"] = split(heads["hip"], fwd_bwd("hip"), max(a.iters, 5))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "fcn_head_ab.jsonl"))
    a = ap.parse_args()
    from mem_amd._lib import require_gpu
    require_gpu()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    for geo in GEOMETRIES:
        row = geometry(*geo, a)
        torch.cuda.empty_cache()
        with open(a.out, "a") as f:
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
