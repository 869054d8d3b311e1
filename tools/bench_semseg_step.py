"""One training step of the reference's segmentation config (mem_224_160k.py): SegModel(EvBEiT ViT-B at 512 x 512, UPerHead,
FCNHead), 16 samples, labels 440 x 640, AdamW with layer decay (mem_amd.run_semseg.SegOptimizer): forward_train + backward +
optimizer step, timed with device events around whole steps; the median over the steps is reported.  One more step runs with
the per-launch timer armed and reports what the attention launches took: a 32 x 32 window (1025 tokens) is none of the shapes
csrc/attn_win.hip serves, so it runs on the streaming family.

    python tools/bench_semseg_step.py [--vit base] [--batch 16] [--steps 8] [--data] [--out profiles/semseg_ab.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vit", default="base")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from mem_amd import ops, run_semseg as R, utils
    args = R.get_args(["--vit", a.vit, "--samples_per_gpu", str(a.batch)])
    torch.manual_seed(0)
    model = R.build_model(args).cuda().train()
    model.backbone.engine
    stream = model.backbone._dp_stream = utils.DropPathStream()
    stream.seed(0)
    groups = R.layer_decay_groups(model, args.num_layers, args.layer_decay_rate, args.lr, args.weight_decay)
    opt = R.SegOptimizer(model, groups, lr=args.lr, betas=tuple(args.betas))
    g = torch.Generator().manual_seed(1)
    img = (torch.rand((a.batch, 3) + tuple(args.net_size), generator=g) * 255).cuda()
    label = torch.randint(0, args.num_classes, (a.batch,) + tuple(args.crop_size), generator=g, dtype=torch.uint8).cuda()

    def step(it):
        R.set_lr(opt, 1500 + it, args)
        key = stream.key()
        model.decode_head.drop_key = model.auxiliary_head.drop_key = key
        losses = model.forward_train(img, label)
        loss = sum(v.float() for k, v in losses.items() if "loss" in k)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    times = []
    for it in range(a.warmup + a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = step(it)
        e1.record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            times.append(e0.elapsed_time(e1))
    T = 1 + (args.net_size[0] // 16) * (args.net_size[1] // 16)
    window = (args.net_size[0] // 16, args.net_size[1] // 16)
    plan = ops.attn_plan(a.batch, T, args.num_heads, window)
    ops.GEMM_TIMER = []
    step(a.warmup + a.steps)
    torch.cuda.synchronize()
    timer, ops.GEMM_TIMER = ops.GEMM_TIMER, None
    attn_f = sum(e0.elapsed_time(e1) for e0, e1, _, code in timer if code == 200)
    attn_b = sum(e0.elapsed_time(e1) for e0, e1, _, code in timer if code == 201)
    rec = {"bench": "semseg_step", "vit": a.vit, "batch": a.batch, "net_size": list(args.net_size), "label": list(args.crop_size),
           "tokens": T, "steps": a.steps, "step_ms": round(statistics.median(times), 2), "step_ms_min": round(min(times), 2),
           "samples_per_s": round(a.batch / statistics.median(times) * 1e3, 1), "loss": round(float(loss.detach()), 4),
           "attn_family": int(plan.family), "attn_family_is_stream": bool(plan.family == ops.ATTN_STREAM),
           "attn_kernels": [k for k, *_ in plan.launches],
           "attn_fwd_ms_per_step": round(attn_f, 2), "attn_bwd_ms_per_step": round(attn_b, 2),
           "attn_share_of_step": round((attn_f + attn_b) / statistics.median(times), 3),
           "note": "the attention figures come from one extra step with per-launch events armed (the side stream is off in it)",
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
