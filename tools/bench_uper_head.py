"""The UPerNet decode head (mem_amd.seg_heads.UPerHead, 4 levels of 768 -> 512 -> 11 at pool scales (1, 2, 3, 6): the reference's
decode head) behind detached input maps, forward + backward (gradients to the four maps and to all 38 parameters), three arms
in one process:

    torch      UPerHead(impl="torch") in fp32 (MIOpen convolutions, torch's pooling, batch norm, interpolate and cat)
    autocast   the same under torch.autocast(bfloat16)
    hip        UPerHead(impl="hip"): the library's bf16 convolution / weight-gradient kernels, csrc/fpn.hip, csrc/ppm.hip and
               csrc/seg_head.hip

at B = 16 on levels of 56 / 28 / 14 / 7 squared (224 x 224 images) and 112 x 160 .. 14 x 20 (440 x 640 images).

Method of tools/bench_psp_head.py (tools/bench_dense_export.py's): the arms alternate inside every repetition, a repetition
times `--iters` back-to-back calls of one arm between two device events, every call takes the next of `--sets` input sets, the
figure is the median over `--reps` repetitions after a warm-up of each arm, with min and max.  The arms get their own copies of
the head (same values).  Peak memory is torch's max_memory_allocated over one more call of each arm on its own, above what was
allocated before it (the hip arm's per-shape buffers exist by then: `hip_buffers_mib` states them).  `hip_library_calls` counts
the calls into libmemhip.so of one forward + backward of the hip arm (a call is one launch, or two where a fold follows; the
kernel launches themselves are a kernel trace's to count).  The timing is reported, not gated: the issue sets no target.

`--only hip` runs nothing but that arm's calls, for a kernel trace of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_uper_head.py --only hip --geometry b16_224

Appends one JSON line per geometry to --out (default profiles/uper_head_ab.jsonl) and prints it.

    python tools/bench_uper_head.py
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

GEOMETRIES = [("b16_224", 16, ((56, 56), (28, 28), (14, 14), (7, 7))), ("b16_440x640", 16, ((112, 160), (56, 80), (28, 40), (14, 20)))]
CIN, C, K, SCALES, L = 768, 512, 11, (1, 2, 3, 6), 4
ARMS = ["torch", "autocast", "hip"]


def flops(B, sizes):
    """forward convolution + data gradient + weight gradient of every convolution: the laterals (1x1), the pyramid's branches
    and bottleneck, the FPN convolutions, fpn_bottleneck and the classifier"""
    R = [B * h * w for h, w in sizes]
    macs = sum(r * CIN * C for r in R[:-1]) + sum(B * s * s for s in SCALES) * CIN * C + R[-1] * 9 * (CIN + len(SCALES) * C) * C
    macs += sum(r * 9 * C * C for r in R[:-1]) + R[0] * 9 * L * C * C + R[0] * C * K
    return 3 * 2.0 * macs


def make_head(impl):
    from mem_amd.seg_heads import UPerHead
    return UPerHead(in_channels=(CIN,) * L, channels=C, num_classes=K, in_index=tuple(range(L)), pool_scales=SCALES, dropout_ratio=0.1,
                    impl=impl).cuda().train()


def arms_of(B, sizes, sets):
    torch.manual_seed(0)
    base = make_head("torch")
    heads = {}
    for arm in ARMS:
        heads[arm] = make_head("hip" if arm == "hip" else "torch")
        heads[arm].load_state_dict(copy.deepcopy(base.state_dict()), strict=True)
    del base
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [[torch.randn((B, CIN, h, w), device="cuda", generator=g).requires_grad_(True) for h, w in sizes] for _ in range(sets)]
    ds = [torch.randn((B, K) + tuple(sizes[0]), device="cuda", generator=g) for _ in range(sets)]

    def fwd_bwd(arm):
        def f(k):
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=arm == "autocast"):
                out = heads[arm](tuple(xs[k % sets]))
            out.backward(ds[k % sets].to(out.dtype))
        return f

    return heads, fwd_bwd


def library_calls(step):
    """the calls into libmemhip.so (kernel entry points: plans and queries left out) of one call of `step`"""
    from mem_amd import ops  # noqa: F401  (declares every entry point on lib)
    from mem_amd._lib import lib
    quiet = ("plan", "workspace", "last_error", "axis_table", "bins", "option", "version", "arch")
    names = [n for n in dir(lib) if n.startswith("memhip_") and not any(q in n for q in quiet)]
    count, real = {}, {n: getattr(lib, n) for n in names}

    def wrap(n):
        def f(*a):
            count[n] = count.get(n, 0) + 1
            return real[n](*a)
        return f

    for n in names:
        setattr(lib, n, wrap(n))
    try:
        step(0)
        torch.cuda.synchronize()
    finally:
        for n in names:
            setattr(lib, n, real[n])
    return count


def geometry(name, B, sizes, a):
    heads, fwd_bwd = arms_of(B, sizes, a.sets)
    res = ab({arm: fwd_bwd(arm) for arm in ARMS}, a.iters, a.reps)
    row = dict(kind="uper_head", geometry=name, B=B, sizes=[list(s) for s in sizes], Cin=CIN, C=C, K=K, pool_scales=list(SCALES),
               what="forward_backward", iters=a.iters, reps=a.reps, sets=a.sets, gflop=round(flops(B, sizes) / 1e9, 2))
    for arm, ts in res.items():
        row[arm] = dict(ms=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3))
    for arm in ARMS:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fwd_bwd(arm)(0)
        torch.cuda.synchronize()
        row[arm]["peak_mib"] = round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)
    calls = library_calls(fwd_bwd("hip"))
    row["hip_library_calls"] = sum(calls.values())
    row["hip_library_calls_by_entry"] = dict(sorted(calls.items()))
    row["hip_buffers_mib"] = round(sum(b.numel() * b.element_size() for b in heads["hip"]._bufs.values()) / 2 ** 20, 1)
    for arm in ARMS[:-1]:
        row["hip_over_" + arm] = round(row["hip"]["ms"] / row[arm]["ms"], 4)
    row["fastest"] = min(ARMS, key=lambda arm: row[arm]["ms"])
    return row


def only(arm, name, B, sizes, a):
    """the calls of one arm and nothing else (a profiler's run): a warm-up, then iters x reps calls"""
    heads, fwd_bwd = arms_of(B, sizes, a.sets)
    step = fwd_bwd(arm)
    for k in range(3):
        step(k)
    torch.cuda.synchronize()
    for k in range(a.iters * a.reps):
        step(k)
    torch.cuda.synchronize()
    print(json.dumps(dict(kind="uper_head_only", arm=arm, geometry=name, calls=a.iters * a.reps, warmup=3)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--geometry", choices=[g[0] for g in GEOMETRIES], default=None)
    ap.add_argument("--only", choices=ARMS, default=None)
    ap.add_argument("--out", default=os.path.join("profiles", "uper_head_ab.jsonl"))
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
