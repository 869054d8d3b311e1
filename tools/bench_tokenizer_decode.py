"""The dVAE tokenizer's decoder (DiscreteVAE.decode, eventvae/vae/vae_model.py:160-171) at the ViT-B tokenizer shape
(oracle/vae_ref.py BASE_VAE: hidden 384, 4 transposed layers, 3 ResBlocks, 224^2), B = 32, three arms in one process:

    hip        HipTokenizer.decode: bf16, csrc/convt.hip + the bf16 convolutions of csrc/conv.hip, chunks of --decode_batch
    torch      the torch module in fp32 (MIOpen)
    autocast   the torch module under torch.autocast(bfloat16)

Method of tools/bench_dense_export.py: the arms alternate inside every repetition, a repetition times `--iters` back-to-back
calls of one arm between two device events (the device is synchronised at the second), every call takes the next of `--sets`
id sets; the figure is the median over `--reps` repetitions after a warm-up of each arm, with min and max (iters x reps >= 20
calls per arm).  TFLOP/s = the FLOP count of the shapes (flops_decode below) over the median.  The timing is reported, not gated.

Appends one JSON line per arm to --out (default profiles/tokenizer_decode_ab.jsonl) and prints it.  Needs the GPU: there is no
fallback.  `--arms hip --reps 3` is the run to put under a kernel trace.

    python tools/bench_tokenizer_decode.py
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_dense_export import ab  # noqa: E402

BASE_VAE = dict(input_H=224, input_W=224, num_tokens=8192, codebook_dim=512, num_layers=4, num_resnet_blocks=3,
                hidden_dim=384, channels=3)       # == oracle/vae_ref.py BASE_VAE (the tool does not import the oracle)


def flops_decode(cfg, B):
    """FLOPs of one decode of B samples, from the shapes: (transposed layers, everything else)."""
    h, w = cfg["input_H"] >> cfg["num_layers"], cfg["input_W"] >> cfg["num_layers"]
    hid, res = cfg["hidden_dim"], cfg["num_resnet_blocks"]
    other = 0.0
    cin = cfg["codebook_dim"]
    if res:
        other += 2.0 * h * w * cin * hid                               # 1x1 behind the codebook
        other += res * 2.0 * h * w * hid * hid * (9 + 9 + 1)           # ResBlock: 3x3, 3x3, 1x1
        cin = hid
    convt = 0.0
    for _ in range(cfg["num_layers"]):                                 # every output pixel: 4 taps x Cin x Cout
        h, w = 2 * h, 2 * w
        convt += 2.0 * h * w * 4 * cin * hid
        cin = hid
    other += 2.0 * h * w * hid * cfg["channels"]                       # final 1x1
    return B * convt, B * other


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--decode_batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--arms", default="hip,torch,autocast")
    ap.add_argument("--out", default=os.path.join("profiles", "tokenizer_decode_ab.jsonl"))
    a = ap.parse_args()
    from mem_amd._lib import require_gpu
    require_gpu()
    from mem_amd.vae_model import DiscreteVAE, HipTokenizer
    torch.manual_seed(0)
    vae = DiscreteVAE(**BASE_VAE).cuda().eval()
    tok = HipTokenizer(vae, max_batch=1, precision="bf16", decode_batch=a.decode_batch)
    g = torch.Generator(device="cuda").manual_seed(1)
    B, n = a.batch, a.sets
    ids = [torch.randint(0, BASE_VAE["num_tokens"], (B, 196), generator=g, device="cuda") for _ in range(n)]

    def torch_arm(autocast):
        def f(k):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                vae.decode(ids[k % n])
        return f
    arms = {"hip": lambda k: tok.decode(ids[k % n]), "torch": torch_arm(False), "autocast": torch_arm(True)}
    arms = {k: arms[k] for k in a.arms.split(",")}
    if "autocast" in arms:
        try:
            arms["autocast"](0)
            torch.cuda.synchronize()
        except RuntimeError as e:
            print("autocast arm not available: %s" % str(e).splitlines()[0])
            del arms["autocast"]
    res = ab(arms, a.iters, a.reps)
    f_t, f_o = flops_decode(BASE_VAE, B)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as f:
        for arm, ts in res.items():
            ms = statistics.median(ts)
            row = dict(kind="tokenizer_decode", arm=arm, B=B, decode_batch=a.decode_batch if arm == "hip" else None,
                       calls=a.iters * a.reps, ms=round(ms, 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3),
                       gflop=round((f_t + f_o) / 1e9, 1), gflop_transposed=round(f_t / 1e9, 1),
                       tflops=round((f_t + f_o) / ms / 1e9, 1), device=torch.cuda.get_device_name(0))
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
