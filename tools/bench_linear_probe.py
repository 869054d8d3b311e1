"""What frozen-backbone probing and forward-only evaluation cost against the full finetuning step: ViT-B/16 at 224^2, 3 input
channels, 101 classes, layer scale 0.1, mean pooling, drop path 0.1, AdamW with layer decay 0.75, synthetic input.  Arms, each on a
fresh model in one process (built, warmed up, timed, freed):

    full     forward, cross-entropy, backward, gradient norm, grouped AdamW at B = 256
    frozen   the same loop after model.freeze_backbone(): forward-only trunk, token pooling, head / fc_norm step
    eval     model.eval() under no_grad at B = 384 (the entrypoint evaluates at 1.5 x the batch size)

Per arm: median over >= 20 steps timed one by one with device events after >= 5 warm-up steps, and the peak of
torch.cuda.max_memory_allocated() over the arm (the statistics are reset once the previous arm is freed).  Prints one JSON line.
A tree without freeze_backbone() (the code before this mode existed) runs the other two arms, so the same file times both sides
of an A/B.

    python tools/bench_linear_probe.py --steps 20 --warmup 5
"""
import argparse
import contextlib
import gc
import io
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(batch, frozen):
    from mem_amd import optim_factory as OF
    from mem_amd.modeling_finetune import ft_vit
    from mem_amd.utils import DropPathStream
    torch.manual_seed(0)
    m = ft_vit(img_size=(224, 224), patch_size=(16, 16), in_chans=3, num_classes=101, embed_dim=768, depth=12, num_heads=12,
               mlp_ratio=4, init_values=0.1, use_mean_pooling=True, use_rel_pos_bias=True, use_abs_pos_emb=False,
               drop_path_rate=0.1, drop_rate=0.0)
    if frozen:
        m.freeze_backbone()
    m = m.cuda().train()
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


def train_step(m, opt, x, y):
    loss = torch.nn.CrossEntropyLoss()(m(x).float(), y)
    loss.backward()
    opt.grad_norm() if hasattr(opt, "grad_norm") else m.engine.grad_norm()
    opt.step()
    opt.zero_grad()
    return loss


def eval_step(m, opt, x, y):
    with torch.no_grad():
        return torch.nn.CrossEntropyLoss()(m(x).float(), y)


def run_arm(name, batch, steps, warmup):
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    m, opt, x, y = build(batch, frozen=name == "frozen")
    fn = train_step
    if name == "eval":
        m.eval()
        fn = eval_step
    for _ in range(warmup):
        fn(m, opt, x, y)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    torch.cuda.synchronize()
    ev[0].record()
    for i in range(steps):
        loss = fn(m, opt, x, y)
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]
    out = {"batch": batch, "ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
           "max_memory_allocated_mb": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1), "loss_finite": bool(torch.isfinite(loss)),
           "stash_allocated": bool(getattr(m.engine, "B_stash", m.engine.B))}
    del m, opt, x, y
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--eval-batch", type=int, default=384)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--arms", default="full,frozen,eval")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    assert a.steps >= 20 and a.warmup >= 5, "median of >= 20 timed steps after >= 5 warm-up steps"
    from mem_amd.modeling_finetune import VisionTransformer
    arms = [k for k in a.arms.split(",") if k != "frozen" or hasattr(VisionTransformer, "freeze_backbone")]
    res = {k: run_arm(k, a.eval_batch if k == "eval" else a.batch, a.steps, a.warmup) for k in arms}
    line = {"metric": "ft_vit ViT-B/16 224^2: full finetuning step, frozen-backbone step, evaluation forward", "tag": a.tag,
            "steps": a.steps, "warmup": a.warmup, "arms": res}
    if "full" in res and "frozen" in res:
        line["frozen_over_full"] = round(res["frozen"]["ms_median"] / res["full"]["ms_median"], 4)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
