"""The two dense-map kernels (csrc/dense.hip) against the torch expressions they replace, and what four exports cost a training
step.  Geometries: ViT-B at B = 256 (14 x 14 = 196 tokens, D = 768) and ViT-L width at B = 64 (30 x 40 = 1200 tokens, D = 1024).

    forward    ops.tokens_to_maps(x)                 vs  x.view(B, T, D)[:, 1:].permute(0, 2, 1).contiguous()
    backward   ops.maps_to_tokens_add(dmap, dx)      vs  dx.view(B, T, D)[:, 1:] += dmap.flatten(2).transpose(1, 2)

Both arms of a pair run in the same process, interleaved: a repetition times `--iters` back-to-back launches of one arm with
device events, then of the other; the figure is the median over `--reps` repetitions after a warm-up of each arm.  Every launch
of a repetition takes the next of `--sets` buffer sets (more bytes than the 256 MB Infinity Cache holds), so the time is HBM
time.  The outputs of the two arms are compared (torch.equal) at the timed size first.  Bytes: 2 * B * L * D * 4 for the
forward (one read, one write), 3 * B * L * D * 4 for the backward (dx is read as well); GB/s = bytes / time, and the fraction
of the 8 TB/s HBM peak.  The run FAILS (exit status 1) when a kernel's median is above its torch expression's.

step: ft_vit ViT-B/16 at 224^2, B = 256, engine level: forward_trunk + backward_trunk(dxl) against the same with
export=(3, 5, 7, 11) and the four map gradients -- 4 + 4 extra launches; alternated step by step, median per arm, difference.

Appends one JSON line per measurement to --out (default profiles/dense_export_ab.jsonl) and prints it.

    python tools/bench_dense_export.py
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
GEOMETRIES = [("vit_b_196", 256, 14, 14, 768), ("vit_l_1200", 64, 30, 40, 1024)]


def timed(fn, iters):
    """Milliseconds per call of fn(k), k = 0 .. iters - 1, between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(iters):
        fn(k)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def ab(arms, iters, reps, warmup=2):
    """arms: {name: fn(k)} -> {name: [ms per call, one per repetition]}, the arms alternating inside every repetition."""
    for fn in arms.values():
        for _ in range(warmup):
            timed(fn, iters)
    out = {n: [] for n in arms}
    for _ in range(reps):
        for n, fn in arms.items():
            out[n].append(timed(fn, iters))
    return out


def kernels(name, B, Hp, Wp, D, a):
    from mem_amd import ops
    L = Hp * Wp
    T = L + 1
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn((B * T, D), device="cuda", generator=g) for _ in range(a.sets)]
    dmaps = [torch.randn((B, D, Hp, Wp), device="cuda", generator=g) for _ in range(a.sets)]
    outs = [torch.empty((B, D, L), device="cuda") for _ in range(a.sets)]
    # the same values on both sides first
    ours = ops.tokens_to_maps(xs[0], B, T, out=outs[0])
    assert torch.equal(ours, xs[0].view(B, T, D)[:, 1:].permute(0, 2, 1).contiguous()), "tokens_to_maps != torch"
    d1, d2 = xs[1].clone(), xs[1].clone()
    ops.maps_to_tokens_add(dmaps[0], d1, B, T)
    d2.view(B, T, D)[:, 1:] += dmaps[0].flatten(2).transpose(1, 2)
    assert torch.equal(d1, d2), "maps_to_tokens_add != torch"
    del d1, d2
    rows = []
    n = a.sets
    fwd = ab({"hip": lambda k: ops.tokens_to_maps(xs[k % n], B, T, out=outs[k % n]),
              "torch": lambda k: xs[k % n].view(B, T, D)[:, 1:].permute(0, 2, 1).contiguous()}, a.iters, a.reps)

    def torch_bwd(k):
        xs[k % n].view(B, T, D)[:, 1:] += dmaps[k % n].flatten(2).transpose(1, 2)
    bwd = ab({"hip": lambda k: ops.maps_to_tokens_add(dmaps[k % n], xs[k % n], B, T), "torch": torch_bwd}, a.iters, a.reps)
    for what, res, passes in (("tokens_to_maps", fwd, 2), ("maps_to_tokens_add", bwd, 3)):
        nbytes = passes * B * L * D * 4
        row = dict(kind="kernel", op=what, geometry=name, B=B, tokens=L, D=D, bytes=nbytes, iters=a.iters, reps=a.reps)
        for arm, ts in res.items():
            med = statistics.median(ts)
            row[arm] = dict(us=round(med * 1e3, 2), us_min=round(min(ts) * 1e3, 2), us_max=round(max(ts) * 1e3, 2),
                            GBps=round(nbytes / (med * 1e-3) / 1e9, 1), hbm_fraction=round(nbytes / (med * 1e-3) / HBM_PEAK, 4))
        row["hip_over_torch"] = round(row["hip"]["us"] / row["torch"]["us"], 4)
        rows.append(row)
    return rows


def step(a):
    from mem_amd.modeling_finetune import ft_vit
    B, idx = 256, (3, 5, 7, 11)
    torch.manual_seed(0)
    m = ft_vit(img_size=(224, 224), patch_size=(16, 16), in_chans=3, num_classes=101, embed_dim=768, depth=12, num_heads=12,
               mlp_ratio=4, init_values=0.1, use_mean_pooling=True, use_rel_pos_bias=True, use_abs_pos_emb=False,
               drop_path_rate=0.0, drop_rate=0.0).cuda().train()
    eng = m.engine
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.rand((B, 3, 224, 224), device="cuda", generator=g)
    dxl = torch.randn((B * eng.T, eng.D), device="cuda", generator=g) * 1e-3
    dmaps = {i: torch.randn((B, eng.D, *eng.window), device="cuda", generator=g) * 1e-3 for i in idx}

    def plain(_k):
        eng.forward_trunk(x)
        eng.backward_trunk(dxl)

    def dense(_k):
        eng.forward_trunk(x, export=idx)
        eng.backward_trunk(dxl, dmaps)
    res = ab({"plain": plain, "dense": dense}, 1, a.steps, warmup=a.warmup)
    mp, md = statistics.median(res["plain"]), statistics.median(res["dense"])
    return dict(kind="step", model="ft_vit ViT-B/16 224^2", B=B, out_indices=list(idx), steps=a.steps,
                plain_ms=round(mp, 3), dense_ms=round(md, 3), added_ms=round(md - mp, 3),
                plain_ms_min_max=[round(min(res["plain"]), 3), round(max(res["plain"]), 3)],
                dense_ms_min_max=[round(min(res["dense"]), 3), round(max(res["dense"]), 3)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "dense_export_ab.jsonl"))
    a = ap.parse_args()
    from mem_amd._lib import require_gpu
    require_gpu()
    rows = []
    for geo in GEOMETRIES:
        rows += kernels(*geo, a)
        torch.cuda.empty_cache()
    if not a.no_step:
        rows.append(step(a))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")
    slower = [(r["op"], r["geometry"]) for r in rows if r["kind"] == "kernel" and r["hip_over_torch"] > 1.0]
    if slower:
        print("FAIL: slower than the torch expression:", slower)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
