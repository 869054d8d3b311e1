"""Which kernels do memhip_attn_fwd / memhip_attn_bwd* launch?  Issues one fixed list of attention calls, once each, so that
two builds can be compared launch for launch under a kernel trace, and each against what ops.attn_plan predicts:

    timeout 600 rocprofv3 --kernel-trace --output-format csv -d OUT_A -- python tools/attn_launch_list.py --tree CHECKOUT_A
    timeout 600 rocprofv3 --kernel-trace --output-format csv -d OUT_B -- python tools/attn_launch_list.py --predict PLAN.json
    python tools/attn_launch_list.py --compare OUT_A OUT_B --plan PLAN.json --out profiles/attn_plan_trace.json

The list: the shapes of the attention tests in tests/test_kernels_gpu.py, ViT-B (197 tokens x 12 heads x B = 256) and ViT-L at
480 x 640 (1201 x 16 x B = 64; B = 16 where the memory does not hold it); forward, and backward with every combination of table
gradient / v_bias gradient / forward output / workspace (none, too small, enough); options attn16 0 / 1 and attn_win 0 / 1 / 2.
--predict (a tree that has ops.attn_plan) also writes the launches the plan names for every call, for the stream's CU count.
--compare writes the three ordered lists of (kernel, grid in workgroups, workgroup, LDS bytes) side by side: identical, or the
first differences."""
import argparse
import csv
import glob
import json
import os
import re
import sys

SHAPES = [(3, 12, (14, 14)), (45, 4, (14, 14)), (2, 2, (4, 4)), (5, 4, (8, 8)), (1, 2, (15, 17)), (40, 3, (4, 9)), (1, 2, (16, 16)),
          (3, 3, (17, 19)), (2, 2, (30, 40)), (64, 16, (17, 17)), (2, 2, (16, 20)), (3, 3, (13, 20)), (4, 3, (7, 40)), (9, 4, (26, 40)),
          (9, 4, (23, 40)), (5, 3, (7, 40)), (29, 3, (14, 14)), (24, 16, (30, 40)), (256, 12, (14, 14)), (64, 16, (30, 40))]
SETTINGS = ((1, 1), (0, 1), (1, 0), (1, 2))         # (attn16, attn_win); the other option stays at its default
STATIC_LDS = {"attn_win_stats_kernel": 2048}          # LDS a kernel declares itself, on top of the dynamic bytes of the plan


def template_args(p, name):
    """The template arguments of launch `name` of AttnPlan p, as the trace prints them."""
    b = ("false", "true")
    return {"attn_fwd_kernel": [p.n], "attn_bwd_kv_kernel": [p.n, b[p.vb]], "attn_bwd_q_kernel": [p.n, b[p.dt]],
            "attn16_bwd_kernel": [b[p.dt], b[p.fd]], "attn_fwd_win_kernel": [p.ww], "attn_bwd_kv_win_kernel": [p.ww, b[p.vb]],
            "attn_bwd_q_win_kernel": [p.ww, b[p.dt]], "attn_bwd_kvs_win_kernel": [p.ww, b[p.vb], b[p.dt]],
            "attn_bwd_qs_win_kernel": [p.ww], "attn_fwd_stream_kernel": [4], "attn_bwd_kv_stream_kernel": [4, b[p.vb]],
            "attn_bwd_q_stream_kernel": [2, b[p.dt]]}.get(name, [])


def predicted(ops, cus, *a, **kw):
    p = ops.attn_plan(*a, stream_cus=cus, **kw)
    return [["%s<%s>" % (n, ",".join(map(str, template_args(p, n)))) if template_args(p, n) else n, list(g), blk,
             lds + STATIC_LDS.get(n, 0)] for n, g, blk, lds in p.launches]


def run(tree, predict):
    sys.path.insert(0, os.path.abspath(tree))
    import torch
    from mem_amd import _lib, ops
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan, n = [], 0
    for B, H, win in SHAPES:
        T, D = win[0] * win[1] + 1, 64 * H
        try:
            z = lambda *sh, dt=torch.float32: torch.zeros(sh, dtype=dt, device="cuda")
            qkv, dout, out = z(B * T, 3 * D, dt=torch.bfloat16), z(B * T, D, dt=torch.bfloat16), z(B * T, D, dt=torch.bfloat16)
            dqkv, lse = z(B * T, 3 * D, dt=torch.bfloat16), z(B, H, ops.attn_tokens_padded(T))
            table, delta = z((2 * win[0] - 1) * (2 * win[1] - 1) + 3, H), z(2 * B * T + 4, H)
            dtable, dqb, dvb = torch.zeros_like(table), z(D), z(D)
            need = ops.attn_bwd_workspace(B, T, H, win)
            spaces = [None] + ([z(1024, dt=torch.uint8), z(need, dt=torch.uint8)] if need else [])
        except torch.OutOfMemoryError:
            assert (B, H, win) == (64, 16, (30, 40)), (B, H, win)
            SHAPES.append((16, 16, (30, 40)))
            continue
        for a16, awin in SETTINGS:
            _lib.set_option("attn16", a16)
            _lib.set_option("attn_win", awin)
            ops.attn_fwd(qkv, B, T, D, H, table, win, out, lse)
            n += 1
            if predict:
                plan += predicted(ops, cus, B, T, H, win)
            for f in range(8):
                dt, dv, o = (dtable if f & 1 else None), (dvb if f & 2 else None), (out if f & 4 else None)
                for ws in spaces:
                    ops.attn_bwd(qkv, dout, lse, delta, table, win, B, T, D, H, 0.125, dqkv, dt, dq_bias=dqb, dv_bias=dv, out=o, ws=ws)
                    n += 1
                    if predict:
                        plan += predicted(ops, cus, B, T, H, win, backward=True, dtable=dt is not None, dv_bias=dv is not None,
                                          out=o is not None, ws=ws)
            _lib.set_option("attn16", 1)
            _lib.set_option("attn_win", 1)
        torch.cuda.synchronize()
        del qkv, dout, out, dqkv, spaces
    if predict:
        json.dump(plan, open(predict, "w"))
    print("%d calls issued on %d CUs" % (n, cus))


def read_trace(d):
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    assert len(files) == 1, (d, files)
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    lds = next(c for c in rows[0] if "LDS" in c.upper())
    out = []
    for r in rows:
        m = re.search(r"(attn\w*_kernel)(<[^>]*>)?", r["Kernel_Name"])
        if not m:
            continue
        wg = [int(r["Workgroup_Size_" + c]) for c in "XYZ"]
        assert wg[1] == wg[2] == 1, r
        # the trace counts work-items: workgroups = grid / workgroup size
        grid = [int(r["Grid_Size_" + c]) // w for c, w in zip("XYZ", wg)]
        args = re.sub(r"\((int|bool)\)|\s", "", m.group(2) or "")
        out.append([m.group(1) + args, grid, wg[0], int(r[lds])])
    return out


def compare(a, b, plan, out):
    lists = {"parent": read_trace(a), "this": read_trace(b), "plan": json.load(open(plan))}
    same = lists["parent"] == lists["this"] == lists["plan"]
    res = {"columns": ["kernel", "grid (workgroups)", "workgroup", "lds_bytes"], "launches": {k: len(v) for k, v in lists.items()},
           "distinct_kernels": {k: len({r[0] for r in v}) for k, v in lists.items()}, "verdict": "identical" if same else "different"}
    if not same:
        rows = zip(*(lists[k] + [None] * 8 for k in ("parent", "this", "plan")))
        res["first_differences"] = [{"index": i, "parent": x, "this": y, "plan": z} for i, (x, y, z) in enumerate(rows)
                                    if not x == y == z][:20]
    else:
        res["kernels"] = sorted({r[0] for r in lists["this"]})
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1)[:4000])
    return 0 if same else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose mem_amd package makes the calls (default: this one)")
    ap.add_argument("--predict", metavar="PLAN.json", help="also write what ops.attn_plan names for every call")
    ap.add_argument("--compare", nargs=2, metavar=("TRACE_PARENT", "TRACE_THIS"))
    ap.add_argument("--plan", metavar="PLAN.json")
    ap.add_argument("--out", default="attn_plan_trace.json")
    args = ap.parse_args()
    sys.exit(compare(args.compare[0], args.compare[1], args.plan, args.out) if args.compare else run(args.tree, args.predict))
