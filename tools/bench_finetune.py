"""Finetuning step time with and without element-wise dropout (ft_vit drop_rate 0 against 0.1), interleaved A/B in one process.

The step of N-Caltech101 finetuning: ViT-B/16 at 224^2, 3 input channels, 101 classes, layer scale 0.1, mean pooling, drop path 0.1
(work skipping, the finetuning default), bf16 engine, AdamW with layer decay 0.75 -- forward, cross-entropy, backward, gradient norm,
grouped AdamW.  Prints one JSON line: median ms/step of each arm over the pairs, and the overhead of dropout.

    python tools/bench_finetune.py --batch 256 --pairs 6 --steps 5
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(drop_rate, batch):
    from mem_amd import optim_factory as OF
    from mem_amd.modeling_finetune import ft_vit
    from mem_amd.utils import DropPathStream
    torch.manual_seed(0)
    m = ft_vit(img_size=(224, 224), patch_size=(16, 16), in_chans=3, num_classes=101, embed_dim=768, depth=12, num_heads=12,
               mlp_ratio=4, init_values=0.1, use_mean_pooling=True, use_rel_pos_bias=True, use_abs_pos_emb=False,
               drop_path_rate=0.1, drop_rate=drop_rate).cuda().train()
    m._dp_stream = DropPathStream()
    m._dp_stream.seed(1)
    depth = len(m.blocks)
    assigner = OF.LayerDecayValueAssigner(list(0.75 ** (depth + 1 - i) for i in range(depth + 2)))
    with contextlib.redirect_stdout(io.StringIO()):
        groups = OF.get_parameter_groups(m, 0.05, m.no_weight_decay(), assigner.get_layer_id, assigner.get_scale)
    opt = OF.FlatAdamW(m, groups, lr=5e-4)
    for gr in opt.param_groups:
        gr["lr"] = 5e-4 * gr["lr_scale"]
    g = torch.Generator().manual_seed(2)
    x = torch.rand((batch, 3, 224, 224), generator=g).cuda()
    y = torch.randint(0, 101, (batch,), generator=g).cuda()
    return m, opt, x, y


def step(m, opt, x, y):
    loss = torch.nn.CrossEntropyLoss()(m(x).float(), y)
    loss.backward()
    m.engine.grad_norm()
    opt.step()
    return loss


def timed(m, opt, x, y, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        step(m, opt, x, y)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--steps", type=int, default=5, help="steps per timed segment")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--drop", type=float, default=0.1)
    a = ap.parse_args()
    arms = {0.0: build(0.0, a.batch), a.drop: build(a.drop, a.batch)}
    for arm in arms.values():
        for _ in range(a.warmup):
            step(*arm)
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for i in range(a.pairs):
        order = list(arms) if i % 2 == 0 else list(arms)[::-1]     # ABBA: neither arm always runs first
        for k in order:
            ms[k].append(timed(*arms[k], a.steps))
    med = {k: statistics.median(v) for k, v in ms.items()}
    loss = {k: float(step(*arm)) for k, arm in arms.items()}
    print(json.dumps({"metric": "ft_vit finetuning step, dropout A/B", "batch": a.batch, "pairs": a.pairs, "steps_per_segment": a.steps,
                      "ms_per_step_drop0": round(med[0.0], 3), "ms_per_step_drop%g" % a.drop: round(med[a.drop], 3),
                      "overhead_frac": round(med[a.drop] / med[0.0] - 1.0, 4),
                      "segments_ms": {str(k): [round(t, 3) for t in v] for k, v in ms.items()},
                      "loss_finite": all(torch.isfinite(torch.tensor(list(loss.values())))).__bool__()}))


if __name__ == "__main__":
    main()
