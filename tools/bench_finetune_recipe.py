"""Cost of the finetuning recipe (mixup / cutmix, soft-target cross-entropy, weight EMA) on the N-Caltech101 finetuning step of
tools/bench_finetune.py (ViT-B/16 at 224^2, B = 256, 101 classes, drop path 0.1, layer decay 0.75), three arms interleaved in one
process (P T H / H T P / ...: no arm always runs first):

    P  the plain step: nn.CrossEntropyLoss, no mixup, no EMA
    T  the recipe as torch ops: x.flip(0) / mul_ / add_ (or the box copy), one-hot targets, sum(-t * log_softmax(x.float())),
       torch._foreach_mul_ / _foreach_add_ over the EMA's parameter views
    H  the recipe through the HIP kernels: mem_amd.mixup.Mixup, loss.SoftTargetCrossEntropy, utils.ModelEma

T and H draw the same parameter sequence (two RandomStates with one seed).  All arms train ONE model (the recipe changes what a
step costs, not the model), and T and H update the same EMA twin.  Prints one JSON line: median ms/step per arm, H - P (the cost
of the recipe), T - H, and the byte floors of the two streaming kernels at 8 TB/s for a kernel trace to be held against.
``--only H`` runs one arm without timing pairs (for `rocprofv3 --kernel-trace --stats -- python tools/bench_finetune_recipe.py --only H`).

    python tools/bench_finetune_recipe.py --batch 256 --pairs 6 --steps 5
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_finetune import build  # noqa: E402

V, DECAY, SMOOTH = 101, 0.9999, 0.1


class TorchRecipe:
    """timm's batch-mode Mixup, SoftTargetCrossEntropy and ModelEma.update written as torch ops (arm T)."""

    def __init__(self, draws, ema):
        self.draws = draws                     # mem_amd.mixup.Mixup used for its host-side draw() only
        self.ema_params = [p.data for _, p in sorted(ema.ema.named_parameters())]
        self.ema = ema

    def mix(self, x, y):
        lam, box = self.draws.draw(x.shape[0], x.shape[2], x.shape[3])
        lam, (yl, yh, xl, xh) = float(lam[0]), (int(v) for v in box[0])
        if yh > yl and xh > xl:
            x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
        elif lam != 1.0:
            x.mul_(lam).add_(x.flip(0).mul_(1.0 - lam))
        off = SMOOTH / V
        y1 = torch.full((y.numel(), V), off, device=x.device).scatter_(1, y.view(-1, 1), 1.0 - SMOOTH + off)
        return x, y1 * lam + y1.flip(0) * (1.0 - lam)

    @staticmethod
    def loss(logits, t):
        return torch.sum(-t * F.log_softmax(logits.float(), dim=-1), dim=-1).mean()

    @torch.no_grad()
    def update(self, model):
        src = [p.data for _, p in sorted(model.named_parameters())]
        torch._foreach_mul_(self.ema_params, DECAY)
        torch._foreach_add_(self.ema_params, src, alpha=1.0 - DECAY)
        self.ema.ema.engine.weights_dirty = True


def make_steps(m, opt, x, y):
    from mem_amd.loss import SoftTargetCrossEntropy
    from mem_amd.mixup import Mixup
    from mem_amd.utils import ModelEma
    ema = ModelEma(m, decay=DECAY)
    ema.ema.engine                                                  # built before anything is timed
    kw = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, label_smoothing=SMOOTH, num_classes=V)
    hip_mix = Mixup(rng=np.random.RandomState(5), **kw)
    torch_recipe = TorchRecipe(Mixup(rng=np.random.RandomState(5), **kw), ema)
    hip_loss = SoftTargetCrossEntropy()
    xs = {k: x.clone() for k in "TH"}                               # mixed in place: each arm keeps its own batch

    def finish(loss):
        loss.backward()
        m.engine.grad_norm()
        opt.step()
        return loss

    def step_p():
        return finish(torch.nn.CrossEntropyLoss()(m(x).float(), y))

    def step_t():
        xm, t = torch_recipe.mix(xs["T"], y)
        loss = finish(torch_recipe.loss(m(xm), t))
        torch_recipe.update(m)
        return loss

    def step_h():
        xm, t = hip_mix(xs["H"], y)
        loss = finish(hip_loss(m(xm), t))
        ema.update(m)
        return loss

    return {"P": step_p, "T": step_t, "H": step_h}, ema


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--pairs", type=int, default=6, help="rounds; each times every arm once, order reversed every other round")
    ap.add_argument("--steps", type=int, default=5, help="steps per timed segment")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["P", "T", "H"], default=None, help="run this arm alone (kernel traces), no comparison")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    m, opt, x, y = build(0.0, a.batch)
    steps, ema = make_steps(m, opt, x, y)
    n_flat = m.engine.nflat
    floors = {"mixup_bytes": 2 * x.numel() * 4, "ema_bytes": 12 * n_flat}
    floors.update({k.replace("bytes", "floor_us_at_8TBps"): round(v / 8e12 * 1e6, 2) for k, v in list(floors.items())})
    if a.only:
        for _ in range(a.warmup + a.steps):
            loss = steps[a.only]()
        torch.cuda.synchronize()
        print(json.dumps({"metric": "finetuning recipe, arm %s alone" % a.only, "steps": a.warmup + a.steps,
                          "loss_finite": bool(torch.isfinite(loss)), **floors}))
        return
    for fn in steps.values():
        for _ in range(a.warmup):
            fn()
    ms = {k: [] for k in steps}
    for i in range(a.pairs):
        for k in (list(steps) if i % 2 == 0 else list(steps)[::-1]):
            ms[k].append(timed(steps[k], a.steps))
    med = {k: statistics.median(v) for k, v in ms.items()}
    finite = all(bool(torch.isfinite(fn())) for fn in steps.values())
    print(json.dumps({"metric": "ft_vit finetuning step: plain (P), recipe as torch ops (T), recipe on HIP kernels (H)",
                      "batch": a.batch, "rounds": a.pairs, "steps_per_segment": a.steps,
                      "ms_per_step": {k: round(v, 3) for k, v in med.items()},
                      "recipe_cost_ms_H_minus_P": round(med["H"] - med["P"], 3),
                      "torch_recipe_cost_ms_T_minus_P": round(med["T"] - med["P"], 3),
                      "H_le_T_on_the_median": bool(med["H"] <= med["T"]),
                      "segments_ms": {k: [round(t, 3) for t in v] for k, v in ms.items()}, "loss_finite": finite, **floors}))


if __name__ == "__main__":
    main()
