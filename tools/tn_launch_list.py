"""Which kernels do the weight-gradient GEMMs of a training step launch?  Prints what ops.gemm_tn_plan names for the products of
a ViT block (proj + qkv and fc2 + fc1 as grouped calls, then each of the four alone), the patch embedding and the token head:
kernel form, grid, reduction grid, workspace bytes, and per product tiles x row slices of how many rows.  Nothing is launched;
with --cus no device is needed.

    python tools/tn_launch_list.py --model base --batch 256 --cus 256
    python tools/tn_launch_list.py --model large --batch 64 --cus 240 --no-workspace      # the atomic forms
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mem_amd import _lib, ops                                             # noqa: E402

KINDS = {ops.TN_128: "gemm_tn_kernel", ops.TN_P8_ATOMIC: "gemm_tn_p8_kernel<atomics>",
         ops.TN_P8_WS: "gemm_tn_p8_kernel<workspace> + tn_reduce_kernel",
         ops.TN_P8_GROUP: "gemm_tn_p8_group_kernel + tn_reduce_group_kernel"}
PTR = 0x10000           # the plan reads the address bits only


def problems(shapes):
    arr = (ops.TnProblem * len(shapes))()
    for q, (R, N, K) in zip(arr, shapes):
        q.A, q.B, q.out, q.lda, q.ldb, q.ldo, q.R, q.N, q.K = PTR, PTR, PTR, N, K, K, R, N, K
    return arr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("base", "large"), default="base")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--cus", type=int, default=None, help="CUs the launch stream may use (default: ask the current device)")
    ap.add_argument("--no-workspace", action="store_true", help="plan without the engine's partial-tile workspace")
    ap.add_argument("--overwrite", action="store_true", help="accumulate = 0 (the first backward of a step)")
    ap.add_argument("--opt", action="append", default=[], metavar="NAME=VALUE", help="tn_p8=0, tn_group=0")
    a = ap.parse_args()
    for o in a.opt:
        name, v = o.split("=")
        _lib.set_option(name, int(v))
    D = {"base": 768, "large": 1024}[a.model]
    M = a.batch * 197
    named = {"proj": (M, D, D), "qkv": (M, 3 * D, D), "fc2": (M, D, 4 * D), "fc1": (M, 4 * D, D),
             "patch_embed": (a.batch * 196, D, 512), "head": (a.batch * 98, 8192, D)}
    calls = [("proj", "qkv"), ("fc2", "fc1")] + [(n,) for n in named]
    print(f"ViT-{a.model}, batch {a.batch}, {'device' if a.cus is None else a.cus} CUs, tn_p8 {_lib.get_option('tn_p8')}, "
          f"tn_group {_lib.get_option('tn_group')}, {'no ' if a.no_workspace else ''}workspace, accumulate {int(not a.overwrite)}")
    for names in calls:
        shapes = [named[n] for n in names]
        ws = None if a.no_workspace else (PTR, 1 << 62)
        print(" + ".join(f"{n} {named[n]}" for n in names))
        for l in ops.gemm_tn_plan(problems(shapes), not a.overwrite, ws, a.cus):
            parts = ", ".join(f"{names[p.problem]}: {p.tiles} tiles x {p.splits} slices of {p.rows_per_split} rows"
                              for p in l.p[:l.count])
            print(f"    {KINDS[l.kind]:50s} grid {l.grid:5d}  reduce {l.reduce_grid:5d}  workspace {l.ws_bytes / 2**20:7.1f} MiB"
                  f"{'  memset' if l.memset_first else ''}{'  atomics' if l.use_atomics else ''}  [{parts}]")


if __name__ == "__main__":
    main()
