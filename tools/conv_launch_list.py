"""Which kernels does HipTokenizer launch for its convolutions?  Prints, per layer of the encoder, what ops.conv_plan names for a
tokenizer config and batch: kernel, grid in workgroups, workgroup size, LDS bytes, and for a dynamic-batch call the range of live
sample counts each of its two launches works for.  Nothing is launched; with --cus no device is needed.

    python tools/conv_launch_list.py --config base --batch 256 --precision fp16x2 --cus 256
    python tools/conv_launch_list.py --config tiny --batch 4 --precision fp32 --dynamic      # the certified mode's recompute
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch import nn                                                      # noqa: E402
from mem_amd import _lib, ops                                             # noqa: E402
from mem_amd.vae_model import DiscreteVAE, ResBlock                       # noqa: E402
from oracle.vae_ref import BASE_VAE, TINY_VAE                             # noqa: E402


def layers(vae):
    """(name, conv, residual, head) in the order HipTokenizer runs them."""
    for i, m in enumerate(vae.encoder):
        if isinstance(m, nn.Sequential):
            yield f"conv{i}", m[0], False, False
        elif isinstance(m, ResBlock):
            for j, c in enumerate((m.net[0], m.net[2], m.net[4])):
                yield f"res{i}.{j}", c, j == 2, False
        else:
            yield "head", m, False, True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=("tiny", "base"), default="base")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--precision", choices=ops.CONV_MODES, default="fp16x2")
    ap.add_argument("--dynamic", action="store_true", help="fp32 only: the plan of a call with n_active (capacity = --batch)")
    ap.add_argument("--cus", type=int, default=None, help="CUs of the device (default: ask the current one)")
    ap.add_argument("--conv-waves", type=int, default=None, help="the conv_waves option (default: the library's)")
    a = ap.parse_args()
    if a.conv_waves is not None:
        _lib.set_option("conv_waves", a.conv_waves)
    vae = DiscreteVAE(**{"tiny": TINY_VAE, "base": BASE_VAE}[a.config])
    h = w = vae.input_H
    print(f"{a.config} tokenizer, batch {a.batch}, {a.precision}{' dynamic' if a.dynamic else ''}, conv_waves {_lib.get_option('conv_waves')}, "
          f"{'device' if a.cus is None else a.cus} CUs")
    for name, c, residual, head in layers(vae):
        f32_out = head and a.precision == "fp16x2"
        p = ops.conv_plan(a.precision, a.batch, h, w, max(4, c.in_channels), c.out_channels, c.kernel_size[0], c.stride[0],
                          c.padding[0], add=residual, out_f32=f32_out, out_padded=not head, dynamic=a.dynamic, device_cus=a.cus)
        for kernel, grid, block, lds, lo, hi in p.launches:
            live = f"  live samples [{lo}, {'inf' if hi == 1 << 30 else hi})" if a.dynamic else ""
            print(f"{name:8s} {h:3d}x{w:<3d} {max(4, c.in_channels):3d} -> {c.out_channels:4d}  k{c.kernel_size[0]} s{c.stride[0]}  M = {p.M:8d}  "
                  f"{kernel:30s} grid {grid:6d} x {block}  lds {lds}{live}")
        h, w = p.Ho, p.Wo


if __name__ == "__main__":
    main()
