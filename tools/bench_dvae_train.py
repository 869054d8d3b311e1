"""One training step of the dVAE tokenizer (eventvae/vae/vae_model.py:184-208 + Adam with clipping, train_vae.py:220,335-337) at
the ViT-B tokenizer shape (oracle/vae_ref.py BASE_VAE: hidden 384, 4 + 4 strided layers, 3 + 3 ResBlocks, 8192 tokens, 224^2),
B = 32, arms in one process:

    hip        vae_train.DVAEEngine.forward_backward + step (bf16 kernels, explicit backward)
    autocast   the torch module's training forward under torch.autocast(bfloat16), autograd, clip_grad_norm_ + Adam
    torch      the same in fp32 (MIOpen), if it runs on the box (the tool says so if it does not)

Method of tools/bench_dense_export.py (`ab`): the arms alternate inside every repetition, a repetition times `--iters`
back-to-back steps between two device events; medians over `--reps` repetitions after a warm-up of each arm, with min / max.
Then, in passes of their own on the same process:
  - the split of the HIP step into its phases (repack, encoder forward, sampling segment, decoder forward, losses, the two
    backward walks, optimizer) and into its leaf kernels (data gradients, conv_wgrad per layer shape, relu_bwd_colsum, the
    gradient layout copies) from the engine's device-event timers, medians over `--reps` steps;
  - conv_wgrad alone per layer shape, alternating with memhip_gemm_bf16_tn at the dense shape with the same (R, N, K) = (pixels,
    channels of small, k*k*C), both in TFLOP/s (2 R N K over the median).
Appends JSON lines to --out (default profiles/dvae_train_ab.jsonl) and prints them.  Needs the GPU: there is no fallback.

    python tools/bench_dvae_train.py
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_dense_export import ab  # noqa: E402

BASE_VAE = dict(input_H=224, input_W=224, num_tokens=8192, codebook_dim=512, num_layers=4, num_resnet_blocks=3,
                hidden_dim=384, channels=3)       # == oracle/vae_ref.py BASE_VAE (the tool does not import the oracle)


def torch_step(vae, opt, img, temp, clip):
    """The reference's training step on the torch module (kl_div in the project's convention: sum over rows / B)."""
    opt.zero_grad(set_to_none=True)
    x = vae.norm(img)
    logits = vae.encoder(x)
    soft = F.gumbel_softmax(logits.float(), tau=temp, dim=1, hard=vae.straight_through)
    sampled = torch.einsum("bnhw,nd->bdhw", soft.to(logits.dtype), vae.codebook.weight.to(logits.dtype))
    out = vae.decoder(sampled)
    loss = vae.loss_fn(x, out.float())
    if vae.kl_div_loss_weight:
        lq = F.log_softmax(logits.float().permute(0, 2, 3, 1).reshape(-1, logits.shape[1]), dim=-1)
        loss = loss + ((lq.exp() * lq).sum() / img.shape[0]) * vae.kl_div_loss_weight
    loss.backward()
    torch.nn.utils.clip_grad_norm_(vae.parameters(), clip)
    opt.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--arms", default="hip,autocast,torch")
    ap.add_argument("--kl_loss_weight", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join("profiles", "dvae_train_ab.jsonl"))
    a = ap.parse_args()
    from mem_amd._lib import require_gpu
    require_gpu()
    from mem_amd import ops
    from mem_amd.vae_model import DiscreteVAE
    from mem_amd.vae_train import DVAEEngine
    torch.manual_seed(0)
    B, temp, clip, lr = a.batch, 0.9, 1e-3, 1e-3
    dev = torch.cuda.get_device_name(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    imgs = [torch.rand(B, 3, 224, 224, generator=g, device="cuda") for _ in range(2)]
    vae = DiscreteVAE(**BASE_VAE, kl_div_loss_weight=a.kl_loss_weight).cuda().train()
    sd = {k: v.clone() for k, v in vae.state_dict().items()}
    eng = DVAEEngine(vae)

    def fresh():
        m = DiscreteVAE(**BASE_VAE, kl_div_loss_weight=a.kl_loss_weight).cuda().train()
        m.load_state_dict(sd)
        return m, torch.optim.Adam(m.parameters(), lr=lr)
    (m16, o16), (m32, o32) = fresh(), fresh()

    def hip(k):
        eng.forward_backward(imgs[k % 2], temp)
        eng.step(lr, max_norm=clip)

    def autocast(k):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            torch_step(m16, o16, imgs[k % 2], temp, clip)
    arms = {"hip": hip, "autocast": autocast, "torch": lambda k: torch_step(m32, o32, imgs[k % 2], temp, clip)}
    arms = {k: arms[k] for k in a.arms.split(",")}
    rows = []
    for name in [n for n in ("autocast", "torch") if n in arms]:
        try:
            arms[name](0)
            torch.cuda.synchronize()
        except RuntimeError as e:
            rows.append(dict(kind="dvae_train_step", arm=name, B=B, ms=None, note="arm does not run on this box: " + str(e).splitlines()[0][:200]))
            del arms[name]
    res = ab(arms, a.iters, a.reps)
    for arm, ts in res.items():
        rows.append(dict(kind="dvae_train_step", arm=arm, B=B, calls=a.iters * a.reps, ms=round(statistics.median(ts), 3),
                         ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), device=dev))
    # ---- the split of the HIP step
    if "hip" in arms:
        phases, leaves = {}, {}
        for r in range(a.reps):
            eng.timers = {}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            hip(r)
            e1.record()
            torch.cuda.synchronize()
            t = eng.timers
            eng.timers = None
            phases.setdefault("step", []).append(e0.elapsed_time(e1))
            marks = t.pop("_marks")
            for (name, ev), (_, nxt) in zip(marks[:-1], marks[1:]):
                if name is not None:
                    phases.setdefault(name, []).append(0.0)
                    phases[name][-1] += ev.elapsed_time(nxt)
            for name, evs in t.items():
                leaves.setdefault(name, []).append((sum(x.elapsed_time(y) for x, y in evs), len(evs)))
        med = lambda v: round(statistics.median(v), 3)
        rows.append(dict(kind="dvae_train_phases", B=B, reps=a.reps, note="device-event spans inside one timed step (the timers add "
                         "events to the stream: the step here is slower than the untimed arm)", ms={k: med(v) for k, v in phases.items()}, device=dev))
        rows.append(dict(kind="dvae_train_leaves", B=B, reps=a.reps, ms={k: med([x for x, _ in v]) for k, v in sorted(leaves.items())},
                         launches={k: v[0][1] for k, v in sorted(leaves.items())}, device=dev))
        # ---- conv_wgrad per layer shape next to memhip_gemm_bf16_tn at the same (R, N, K)
        hid, T, cp = 384, 8192, 512
        shapes, h = [], 224
        for i in range(4):
            h //= 2
            if i == 0:
                shapes.append((4, 2, 1, h, 4, hid, True))
            shapes.append((4, 2, 1, h, hid, hid, True))
        shapes += [(3, 1, 1, 14, hid, hid, True), (1, 1, 0, 14, hid, hid, True), (1, 1, 0, 14, hid, T, False), (1, 1, 0, 14, cp, hid, True),
                   (1, 1, 0, 224, hid, 8, False)]
        for k, s, p, hs, C_, N, padded in shapes:
            M, K = B * hs * hs, k * k * C_
            small = torch.randn((B, hs + 2, hs + 2, N) if padded else (M, N), generator=g, device="cuda").bfloat16()
            big = torch.zeros((B, s * hs + 2, s * hs + 2, C_), dtype=torch.bfloat16, device="cuda")
            big[:, 1:-1, 1:-1] = torch.randn((B, s * hs, s * hs, C_), generator=g, device="cuda").bfloat16()
            grad = torch.empty((N, K), device="cuda")
            plan = ops.conv_wgrad_plan(B, hs, hs, C_, N, k, s, p, small_padded=padded)
            ws = torch.empty(max(plan.ws_bytes // 4, 1), device="cuda")
            A, Bm = torch.randn((M, N), generator=g, device="cuda").bfloat16(), torch.randn((M, K), generator=g, device="cuda").bfloat16()
            tnb = ops.gemm_tn_workspace(M, N, K)
            tws = torch.empty(tnb, dtype=torch.uint8, device="cuda") if tnb else None
            out = torch.empty((N, K), device="cuda")
            two = ab({"conv_wgrad": lambda _: ops.conv_wgrad(small, big, grad, B, hs, hs, C_, N, k, s, p, small_padded=padded,
                                                              workspace=ws if plan.ws_bytes else None),
                      "gemm_tn": lambda _: ops.gemm_tn(A, Bm, M, N, K, out, accumulate=False, workspace=tws)}, 4, a.reps)
            fl = 2.0 * M * N * K
            ms = {n: statistics.median(v) for n, v in two.items()}
            rows.append(dict(kind="conv_wgrad_layer", form=[k, s, p], B=B, Hs=hs, C=C_, N=N, small_padded=padded, R=M, K=K, splits=plan.splits,
                             grid=plan.grid, ms=round(ms["conv_wgrad"], 4), tflops=round(fl / ms["conv_wgrad"] / 1e9, 1),
                             gemm_tn_ms=round(ms["gemm_tn"], 4), gemm_tn_tflops=round(fl / ms["gemm_tn"] / 1e9, 1), device=dev))
            del small, big, A, Bm
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as f:
        for row in rows:
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
