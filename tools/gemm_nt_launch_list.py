"""Which kernels does memhip_gemm_bf16_nt launch?  Issues one fixed list of NT GEMM calls, once each, so that two builds can
be compared launch for launch under a kernel trace:

    rocprofv3 --kernel-trace --output-format csv -d OUT_A -- python tools/gemm_nt_launch_list.py --tree CHECKOUT_A
    rocprofv3 --kernel-trace --output-format csv -d OUT_B -- python tools/gemm_nt_launch_list.py
    python tools/gemm_nt_launch_list.py --compare OUT_A OUT_B --out profiles/gemm_nt_plan_trace.json

The list: the worked shapes of tests/test_gemm_plan_cpu.py, the shapes of test_gemm_dispatch_fuzz_exact, the Linear shapes of
ViT-B at batch 256 and ViT-L at batch 64; every epilogue valid for the shape (RESIDUAL with and without the bf16 branch
copy); default options and the settings of tools/resid_gemm_probe.py / tools/rem_probe.py.  --compare reads the two traces and
writes the ordered lists of (kernel, grid, workgroup, LDS bytes) of the GEMM kernels side by side: identical, or the diff."""
import argparse
import csv
import glob
import json
import os
import sys

SETTINGS = ({}, {"gemm_p8_pair": 0}, {"gemm_p8_half": 0}, {"gemm_p8": 0}, {"gemm_p8": 0, "gemm256": 0}, {"gemm_split": 0})


def shapes():
    import numpy as np
    rng = np.random.default_rng(123)
    fuzz = [(int(rng.integers(1, 9000)), 8 * int(rng.integers(1, 200)), 64 * int(rng.integers(1, 20))) for _ in range(14)]
    fuzz += [(4096, 256, 128), (4095, 1024, 192), (12289, 1024, 1024), (19216, 4096, 1024), (19216, 1024, 4096),
             (8193, 768, 64), (50432, 256, 128), (4097, 3072, 320), (4224, 512, 128)]
    worked = [(50432, 768, 768), (50432, 2304, 768), (4196, 768, 768), (4095, 1024, 192), (8193, 768, 64), (4097, 3072, 320),
              (50432, 768, 512), (4352, 4096, 128)]
    vit_b = [(256 * 197, n, k) for n, k in ((2304, 768), (768, 768), (3072, 768), (768, 3072))]
    vit_l = [(64 * 197, n, k) for n, k in ((3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096))]
    out = []
    for s in worked + fuzz + vit_b + vit_l:
        if s not in out:
            out.append(s)
    return out


def run(tree):
    sys.path.insert(0, os.path.abspath(tree))
    import torch
    from mem_amd import _lib, ops
    n = 0
    for M, N, K in shapes():
        z = lambda *sh, dt=torch.float32: torch.zeros(sh, dtype=dt, device="cuda")
        A, B = z(M, K, dt=torch.bfloat16), z(N, K, dt=torch.bfloat16)
        o32, x, xin = z(M, N), z(M + 1, N), z(M, N)
        o0, o1, h = z(M, N, dt=torch.bfloat16), z(M, N, dt=torch.bfloat16), z(M, N, dt=torch.bfloat16)
        dg = z(M, N, dt=torch.float16)
        bias, vec, keep, mask = z(N), z(N), z(M // 197 + 2) + 1.0, z(M, dt=torch.uint8)
        smap = torch.arange(M // 197 + 2 + 256, dtype=torch.int32, device="cuda")
        drop = ops.dropout_params(1, 2, 3, 0.1)
        calls = [
            (ops.EPI_BIAS_BF16, dict(out0=o0, bias=bias)),
            (ops.EPI_BIAS_GELU, dict(out0=o0, out1=o1, bias=bias)),
            (ops.EPI_RESIDUAL, dict(bias=bias, vec1=vec, resid=x, aux=xin, ldaux=N, rows_per_sample=197)),
            (ops.EPI_RESIDUAL, dict(out0=o0, bias=bias, vec1=vec, resid=x, rowmask=keep, keep_prob=0.9, rows_per_sample=197)),
            (ops.EPI_RESIDUAL, dict(bias=bias, vec1=vec, resid=x, aux=xin, ldaux=N, sample_map=smap, keep_prob=0.9, rows_per_sample=197)),
            (ops.EPI_DGELU, dict(out0=o0, aux=h)),
            (ops.EPI_F32, dict(out0=o32)),
            (ops.EPI_PATCH_EMBED, dict(bias=bias, vec1=vec, resid=x, aux=mask, rows_per_sample=M)),
            (ops.EPI_BIAS_GELU_DG, dict(out0=dg, out1=o1, bias=bias)),
            (ops.EPI_MUL_AUX, dict(out0=o0, aux=dg)),
            (ops.EPI_RESIDUAL_DROP, dict(bias=bias, vec1=vec, resid=x, aux=xin, ldaux=N, rows_per_sample=197, dropout=drop)),
        ]
        for opts in SETTINGS:
            for name, v in opts.items():
                _lib.set_option(name, v)
            for epi, kw in calls:
                ops.gemm_nt(A, B, M, N, K, epi, **kw)
                n += 1
            for name in opts:
                _lib.set_option(name, 1)
        torch.cuda.synchronize()
    print("%d calls issued" % n)


def read_trace(d):
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    assert len(files) == 1, (d, files)
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    lds = next(c for c in rows[0] if "LDS" in c.upper())
    return [(r["Kernel_Name"], int(r["Grid_Size_X"]), int(r["Workgroup_Size_X"]), int(r[lds]))
            for r in rows if any(k in r["Kernel_Name"] for k in ("gemm_nt_kernel", "gemm256_kernel", "gemm_p8_"))]


def compare(a, b, out):
    la, lb = read_trace(a), read_trace(b)
    res = {"launches_a": len(la), "launches_b": len(lb), "distinct_kernels_a": len({r[0] for r in la}),
           "distinct_kernels_b": len({r[0] for r in lb}), "columns": ["kernel", "grid", "workgroup", "lds_bytes"],
           "verdict": "identical" if la == lb else "different"}
    if la != lb:
        res["first_differences"] = [{"index": i, "a": x, "b": y} for i, (x, y) in enumerate(zip(la, lb)) if x != y][:20]
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1)[:3000])
    return 0 if la == lb else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose mem_amd package makes the calls (default: this one)")
    ap.add_argument("--compare", nargs=2, metavar=("TRACE_A", "TRACE_B"))
    ap.add_argument("--out", default="gemm_nt_plan_trace.json")
    args = ap.parse_args()
    sys.exit(compare(args.compare[0], args.compare[1], args.out) if args.compare else run(args.tree))
