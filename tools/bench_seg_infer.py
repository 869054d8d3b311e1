"""The end of segmentation inference -- the logits of V views to a label map -- two arms in one process:

    hip     mem_amd.ops.seg_predict: one gather kernel (csrc/seg_predict.hip), nothing upsampled in memory
    torch   the same arithmetic as torch ops on the device in fp32, as mmseg 0.30 writes it: per view F.interpolate(bilinear) ->
            preds += F.pad(...) and count_mat += 1 -> preds / count_mat -> softmax -> flip -> mean over the passes -> argmax

at B = 16, C = 11, logits 128 x 128, canvas 440 x 640: whole image, whole image with the flipped pass, and sliding windows
(crop 256 x 256, stride 171 x 171: 12 windows) with the flipped pass.

Method: the arms alternate inside every repetition; a repetition times `--iters` back-to-back calls of one arm with the host
clock between two device synchronisations; every call takes the next of `--sets` input sets; the figure is the median over
`--reps` repetitions after a warm-up of each arm, with min and max.  Per arm also the peak of allocated device memory above
what is allocated before one call (inputs and the label map excluded).  The timing is reported, not gated.  First the two arms
must agree: every label equal where the torch arm's top-2 margin is at least 1e-5.

Appends one JSON line per shape to --out (default profiles/seg_infer_ab.jsonl) and prints it.

    python tools/bench_seg_infer.py
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, C, HW, CANVAS = 16, 11, (128, 128), (440, 640)
SHAPES = [("whole", None, None, False), ("whole_flip", None, None, True), ("slide_256_171_flip", (256, 256), (171, 171), True)]


def torch_arm(logits, rects, window, canvas):
    """-> (pred u8 [B, H, W], P)"""
    (H, W), (hc, wc) = canvas, window
    passes = sorted({f for _, _, f in rects})
    total = None
    for f in passes:
        preds = logits.new_zeros((logits.shape[1], logits.shape[2], H, W))
        count = logits.new_zeros((1, 1, H, W))
        for v, (y1, x1, vf) in enumerate(rects):
            if vf != f:
                continue
            up = F.interpolate(logits[v], size=(hc, wc), mode="bilinear", align_corners=False)
            preds += F.pad(up, (x1, W - x1 - wc, y1, H - y1 - hc))
            count[:, :, y1:y1 + hc, x1:x1 + wc] += 1
        P = F.softmax(preds / count, dim=1)
        if f:
            P = P.flip(3)
        total = P if total is None else total + P
    P = total / len(passes)
    return P.argmax(dim=1).to(torch.uint8), P


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(iters):
        fn(k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def shape(name, crop, stride, flip, a):
    from mem_amd import ops
    from mem_amd.seg_infer import slide_windows
    H, W = CANVAS
    window = crop or CANVAS
    wins = slide_windows(CANVAS, crop, stride) if crop else [(0, 0)]
    rects = [(y, x, f) for f in ((0, 1) if flip else (0,)) for y, x in wins]
    V = len(rects)
    g = torch.Generator(device="cuda").manual_seed(1)
    sets = [torch.randn((V, B, C) + HW, device="cuda", generator=g) * 3 for _ in range(a.sets)]
    pred = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
    arms = {"hip": lambda k: ops.seg_predict(sets[k % a.sets], rects, window, CANVAS, pred=pred),
            "torch": lambda k: torch_arm(sets[k % a.sets], rects, window, CANVAS)[0]}
    # the same labels first, then the clock
    want, P = torch_arm(sets[0], rects, window, CANVAS)
    top = torch.topk(P, 2, dim=1).values
    sure = (top[:, 0] - top[:, 1]) >= 1e-5
    got = arms["hip"](0)
    torch.cuda.synchronize()
    differing = int((got[sure] != want[sure]).sum())
    assert differing == 0, (name, differing)
    row = dict(kind="seg_infer", shape=name, B=B, C=C, h=HW[0], w=HW[1], H=H, W=W, views=V, window=list(window), iters=a.iters,
               reps=a.reps, sets=a.sets, below_margin=int((~sure).sum()), upsampled_mb_per_view=round(B * C * window[0] * window[1] * 4 / 1e6, 1))
    del want, P, top, sure, got
    for fn in arms.values():
        for _ in range(2):
            timed(fn, a.iters)
    ts = {n: [] for n in arms}
    for _ in range(a.reps):
        for n, fn in arms.items():
            ts[n].append(timed(fn, a.iters))
    for n, t in ts.items():
        row[n] = dict(ms=round(statistics.median(t), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4))
    for n, fn in arms.items():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn(0)
        torch.cuda.synchronize()
        row[n]["peak_mb"] = round((torch.cuda.max_memory_allocated() - before) / 1e6, 1)
    row["hip_over_torch"] = round(row["hip"]["ms"] / row["torch"]["ms"], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "seg_infer_ab.jsonl"))
    a = ap.parse_args()
    from mem_amd._lib import require_gpu
    require_gpu()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    for s in SHAPES:
        row = shape(*s, a)
        torch.cuda.empty_cache()
        line = json.dumps(row)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
