#!/usr/bin/env python
"""bench.py -- MEM pretraining throughput on MI355X (BASELINE.json metric: pretrain samples/sec,
ViT-B/16, 224^2 2-bin event voxels, bf16, B=256 per GPU).

One "step" = one pass of the hot path over one synthetic batch that is already resident in HBM:
  events f64 (N,4) x256 -> fused augment+rasterize -> fused event_norm -> block-wise masks (host
  MT19937, overlapped) -> ViT-B masked forward + CE -> backward (RCCL all-reduce overlapped when
  N>1) -> grad-norm/clip + AdamW.
Launch:  python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
  A plain run measures the headline only: set-up, W warm-up steps, K timed steps, the outputs of the last timed step when
  --dump-outputs is given, the JSON line.  --full adds everything else the line can carry (per-GEMM HIP-event roofline,
  speed of light, tokenizer / entrypoint / rasterizer / config #4 / config #5 figures, the CPU baseline, and for N > 1 the
  steps without the gradient exchange); each of those can still be left out of a --full run with its --no-* switch.
  --dump-outputs DIR: after the run, the last timed step's batch goes through the training step once more, from the state the
  run started from, and what that step computed is written as DIR/<name>.npy (float32; fixed, seeded samples of the large
  arrays, ~20 MB in all).  Inputs and starting state are seeded, so every run with the same arguments writes the same
  arrays up to rounding (replay_last_step says why not the last timed step's own state), and two builds can be compared
  output for output.
  N>1, either form works:
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N ...                (the driver's form: RANK / LOCAL_RANK / WORLD_SIZE come from the env)
    python bench.py --gpus N ...             (self-launching: with no WORLD_SIZE in the env this process starts
        exactly that torchrun command as a CHILD before anything touches the GPU, relays its output, prints rank 0's
        JSON line last and exits with the child's return code -- no exec of a GPU-initialised process)
Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FLOP_PER_SAMPLE = {2: 108.85e9, 3: 109.08e9}      # BASELINE.md section 2 (GEMMs only, fwd+bwd)
TIMER_EVERY = 32                                   # one timed step in 32 carries the per-GEMM HIP events (see timer_steps)
POST_REGION_TIMER_STEPS = 4                        # instrumented steps run right behind the timed region (pooled with the ones inside)


def timer_steps(k):
    """Timed steps that carry the per-GEMM HIP events: the 5th, then every 32nd (K = 20 -> one step, K = 100 -> three).
    An instrumented step runs its weight-gradient GEMMs on the launch stream (the events need a stream order) and costs
    ~5 ms more than a plain one -- it is inside the timed region, so it is kept rare."""
    return set(range(min(k - 1, 4), k, TIMER_EVERY))
PEAK_BF16_TFLOPS = 2500.0                          # MI355X dense bf16 (MI355X_MICROARCH.md)


def executed_flop_per_sample(eng, C):
    """GEMM FLOPs per sample the engine EXECUTED in the step it just ran (same 2*M*N*K accounting as FLOP_PER_SAMPLE,
    BASELINE.md section 2): a stochastic-depth branch runs on its kept samples only (work skipping), the last block's MLP
    on the rows that reach the head (tail rows).  The reference's count has every sample in every branch."""
    T, D, Hd, L, V = eng.T, eng.D, eng.hidden, eng.L, eng.V
    B, M, Mm = eng.cur["B"], eng.cur["M"], eng.cur["Mm"]
    attn = 2.0 * T * D * 3 * D + 2.0 * T * D * D + 2 * 2.0 * T * T * D          # qkv, proj, QK^T, PV
    mlp = 2 * 2.0 * T * D * Hd
    plan = eng.cur.get("plan")
    tot = 2.0 * L * eng.Kpe * D + 2.0 * (Mm / B) * D * V                         # patch embedding, lm_head on the masked rows
    for i in range(eng.depth):
        ka = km = 1.0
        if plan is not None:
            if plan["n"][2 * i] is not None:
                ka = plan["n"][2 * i] / B
            if plan["n"][2 * i + 1] is not None:
                km = plan["n"][2 * i + 1] / B
        if i == eng.depth - 1 and eng.cur.get("tail") is not None:
            km = Mm / float(M)                                                   # every sample, its masked rows only
        tot += ka * attn + km * mlp
    return 3.0 * tot


# ---- readers of the committed PMC summaries (profiles/*.json).  Each returns None when the file or a key is missing:
# a changed layout must show up as a failing CPU test (tests/test_bench_profiles.py), not as a lost figure at run time.
def _load_profile(name):
    path = os.path.join(ROOT, "profiles", name)
    if not os.path.exists(path):
        return None
    with open(path) as f:
        return json.load(f)


def raster_traffic_per_sample(tj=None):
    """HBM bytes per sample of the long-stream rasterizer (raster_bin_keys + raster_bin_accum) from
    profiles/raster_traffic.json = tools/prof_pmc_raster.sh: per-kernel {hbm_bytes_per_launch}, one launch =
    `_meta.samples_per_launch` samples of 1 M events (64 when the file carries no _meta: tools/raster_bench.py)."""
    tj = _load_profile("raster_traffic.json") if tj is None else tj
    if not tj:
        return None
    per_launch = 0
    for k in ("raster_bin_keys", "raster_bin_accum"):
        if k not in tj or "hbm_bytes_per_launch" not in tj[k]:
            return None
        per_launch += tj[k]["hbm_bytes_per_launch"]
    return per_launch / float(tj.get("_meta", {}).get("samples_per_launch", 64))


def gemm_traffic_per_launch(kernel, tj=None):
    tj = _load_profile("gemm_traffic.json") if tj is None else tj
    return (tj or {}).get(kernel, {}).get("hbm_bytes_per_launch")


def wgrad_traffic_per_product(tj=None):
    """HBM bytes per weight-gradient PRODUCT from the PMC passes: the single launches (gemm_tn_p8_kernel, one product) and the
    grouped launches of the engine (gemm_tn_p8_group_kernel, two products each: proj + qkv, fc2 + fc1), weighted by their
    launch counts in that profile; None until collected."""
    tj = _load_profile("gemm_traffic.json") if tj is None else tj
    one, grp = (tj or {}).get("gemm_tn_p8_kernel"), (tj or {}).get("gemm_tn_p8_group_kernel")
    if not one and not grp:
        return None
    byts = sum(e["hbm_bytes_per_launch"] * e["launches"] for e in (one, grp) if e)
    prods = (one["launches"] if one else 0) + 2 * (grp["launches"] if grp else 0)
    return round(byts / prods)


def wgrad_kernel_split(sj=None):
    """Per weight-gradient PRODUCT, from the committed rocprofv3 --stats summary of the sequential step (profiles/wgrad_split.json,
    written by tools/r06_collect.py from r06_final_seq_kernel_stats.csv): microseconds in the GEMM kernel (single + grouped
    launches) and in its reduction pass, and the fraction of the 2.5 PFLOP/s peak of the kernel alone / with the reduction."""
    sj = _load_profile("wgrad_split.json") if sj is None else sj
    if not sj or "kernel_us_per_product" not in sj:
        return None
    return {k: sj[k] for k in ("kernel_us_per_product", "reduction_us_per_product", "frac_kernel_alone", "frac_with_reduction",
                               "products", "source") if k in sj}


def mfma_util_by_kernel(uj=None):
    uj = _load_profile("mfma_util.json") if uj is None else uj
    if not uj:
        return None
    return {k.lstrip("_"): v["mfma_util"] for k, v in uj.items() if isinstance(v, dict) and "mfma_util" in v}


def kernel_clock(cj=None):
    """In-kernel shader clock of the GEMM main loops from profiles/r05_clock.json (tools/clock_probe.py: stamp build,
    d(s_memtime) / d(s_memrealtime) x 100 MHz after 2 s of back-to-back launches): {"gemm_p8_ghz", "gemm_tn_p8_ghz",
    "at_clock_peak_tflops", ...} or None.  The dense bf16 peak the chip can issue at that clock is 2.5 PFLOP/s x clock / 2.4."""
    src = "r06_clock.json"
    if cj is None:
        cj = _load_profile(src)
        if cj is None:
            src = "r05_clock.json"
            cj = _load_profile(src)
    if not cj or "kernels" not in cj:
        return None
    nt = [v["clock_ghz"] for k, v in cj["kernels"].items() if k.startswith("gemm_p8 ")]
    tn = [v["clock_ghz"] for k, v in cj["kernels"].items() if k.startswith("gemm_tn_p8 ")]
    if not nt or not tn:
        return None
    nt_g, tn_g = sum(nt) / len(nt), sum(tn) / len(tn)
    return {"gemm_p8_ghz": round(nt_g, 3), "gemm_tn_p8_ghz": round(tn_g, 3), "spec_clock_ghz": cj.get("spec_clock_ghz", 2.4),
            "at_clock_peak_tflops": round(PEAK_BF16_TFLOPS * min(nt_g, tn_g) / cj.get("spec_clock_ghz", 2.4), 1),
            "spec_peak_tflops": PEAK_BF16_TFLOPS, "source": "profiles/" + src + " (tools/clock_probe.py; " + cj.get("method", "") + ")"}


DUMP_SAMPLE = 1 << 20                              # --dump-outputs: elements kept of a larger array (4 MB in float32)


def dump_outputs(out_dir, arrays):
    """--dump-outputs: device tensors -> out_dir/<name>.npy in float32.  An array of more than DUMP_SAMPLE elements is
    written as a fixed sample of them: DUMP_SAMPLE flat indices drawn by a generator seeded from the name, in ascending
    order -- the same elements in every run and every build.  Returns {name: [shape written, elements of the array]}."""
    import zlib
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    info = {}
    for name, t in sorted(arrays.items()):
        flat = t.detach().reshape(-1)
        n = flat.numel()
        if n > DUMP_SAMPLE:
            idx = np.sort(np.random.default_rng(zlib.crc32(name.encode())).integers(0, n, DUMP_SAMPLE))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        v = flat.float().cpu().numpy()
        if n <= DUMP_SAMPLE:
            v = v.reshape(tuple(t.shape))
        np.save(os.path.join(out_dir, name + ".npy"), v)
        info[name] = [list(v.shape), n]
    return info


HBM_ACHIEVABLE_TBS = 6.3                           # MI355X_MICROARCH.md: 8.0 TB/s spec, 6.29 measured (float4 copy)


def speed_of_light(eng, hw, events_per_sample, at_clock_peak_tflops, ms_per_step):
    """The floor of the step the engine just ran, launch by launch: max(algorithmic FLOPs / the MFMA peak AT THE CLOCK the chip holds
    under the GEMM main loops, algorithmic HBM bytes / 6.3 TB/s achievable), every tensor a launch must read or write counted
    once, summed per kernel family with NO overlap between launches (a sequential floor; the two-stream step can go below a
    family's share, never below max(sum of MFMA floors, sum of HBM floors)).  Rows follow DESIGN.md section 4; block-level
    launches count the samples stochastic depth kept and the last block's MLP the rows that reach the head, as executed."""
    T, D, Hd, Lp, V = eng.T, eng.D, eng.hidden, eng.L, eng.V
    B, M, Mm = eng.cur["B"], eng.cur["M"], eng.cur["Mm"]
    plan = eng.cur.get("plan")
    pk, bw = at_clock_peak_tflops * 1e12, HBM_ACHIEVABLE_TBS * 1e12
    fam = {}

    def add(name, flops, byts, n=1.0):
        f = fam.setdefault(name, {"launches": 0.0, "flop": 0.0, "bytes": 0.0, "mfma_ms": 0.0, "hbm_ms": 0.0, "floor_ms": 0.0})
        tf, tb = flops / pk * 1e3, byts / bw * 1e3
        f["launches"] += n; f["flop"] += n * flops; f["bytes"] += n * byts
        f["mfma_ms"] += n * tf; f["hbm_ms"] += n * tb; f["floor_ms"] += n * max(tf, tb)

    def nt(name, m, n, k, extra_bytes):          # NT GEMM [m,k] x [n,k]^T: bf16 operands once + what the epilogue moves
        add(name, 2.0 * m * n * k, 2.0 * m * k + 2.0 * n * k + extra_bytes)

    def tn(name, r, n, k):                       # weight gradient [n,k] += sum_r dY[r,n] X[r,k]: operands once, fp32 result once
        add(name, 2.0 * r * n * k, 2.0 * r * (n + k) + 4.0 * n * k)

    # event path + patch embedding
    Hh, Ww = hw
    add("rasterize + event_norm (HBM)", 0.0, B * (32.0 * events_per_sample + 3.0 * Hh * Ww) + B * 10.0 * Hh * Ww)
    nt("patch embedding GEMMs (fwd + wgrad)", B * Lp, D, eng.Kpe, 2.0 * B * Lp * eng.Kpe + 4.0 * M * D)
    tn("patch embedding GEMMs (fwd + wgrad)", B * Lp, D, eng.Kpe)
    for i in range(eng.depth):
        ka = km = 1.0
        if plan is not None:
            if plan["n"][2 * i] is not None:
                ka = plan["n"][2 * i] / B
            if plan["n"][2 * i + 1] is not None:
                km = plan["n"][2 * i + 1] / B
        ma, mm_ = M * ka, M * km
        if i == eng.depth - 1 and eng.cur.get("tail") is not None:
            mm_ = float(Mm)
        # ---- forward
        add("LayerNorm forward (HBM)", 0.0, 6.0 * ma * D)                                  # fp32 in, bf16 out
        nt("NT GEMMs, bf16 / GELU epilogues", ma, 3 * D, D, 2.0 * ma * 3 * D)              # qkv
        add("attention forward", 4.0 * T * T * D * B * ka, 2.0 * ma * 3 * D + 2.0 * ma * D)
        nt("NT GEMMs, fp32 residual epilogue", ma, D, D, 8.0 * ma * D)                     # proj: x read + x written (fp32)
        add("LayerNorm forward (HBM)", 0.0, 6.0 * mm_ * D)
        nt("NT GEMMs, bf16 / GELU epilogues", mm_, Hd, D, 4.0 * mm_ * Hd)                  # fc1: GELU out bf16 + stored derivative fp16
        nt("NT GEMMs, fp32 residual epilogue", mm_, D, Hd, 8.0 * mm_ * D)                  # fc2
        # ---- backward
        nt("NT GEMMs, bf16 / GELU epilogues", mm_, Hd, D, 4.0 * mm_ * Hd)                  # fc2 dgrad x stored derivative
        tn("weight-gradient GEMMs", mm_, D, Hd)
        nt("NT GEMMs, bf16 / GELU epilogues", mm_, D, Hd, 2.0 * mm_ * D)                   # fc1 dgrad
        tn("weight-gradient GEMMs", mm_, Hd, D)
        add("LayerNorm backward + branch backward (HBM)", 0.0, 16.0 * mm_ * D)             # 3 fp32 streams + 2 bf16
        nt("NT GEMMs, bf16 / GELU epilogues", ma, D, D, 2.0 * ma * D)                      # proj dgrad
        tn("weight-gradient GEMMs", ma, D, D)
        add("attention backward", 10.0 * T * T * D * B * ka, 2.0 * ma * 3 * D * 2 + 2.0 * ma * D * 2)
        nt("NT GEMMs, bf16 / GELU epilogues", ma, D, 3 * D, 2.0 * ma * D)                  # qkv dgrad
        tn("weight-gradient GEMMs", ma, 3 * D, D)
        add("LayerNorm backward + branch backward (HBM)", 0.0, 16.0 * ma * D)
    # head: final norm on the masked rows, lm_head, CE (logits bf16 read, dlogits written in place), dgrad + wgrad
    add("LayerNorm forward (HBM)", 0.0, 6.0 * Mm * D)
    nt("NT GEMMs, bf16 / GELU epilogues", Mm, V, D, 2.0 * Mm * V)
    add("cross entropy (HBM)", 0.0, 4.0 * Mm * V)
    nt("NT GEMMs, bf16 / GELU epilogues", Mm, D, V, 2.0 * Mm * D)
    tn("weight-gradient GEMMs", Mm, V, D)
    add("LayerNorm backward + branch backward (HBM)", 0.0, 14.0 * Mm * D)
    # optimizer: gradient norm (4 B / parameter), AdamW (p, g, m, v read; p, m, v written), bf16 shadow + transposed matrices
    add("grad norm + AdamW + bf16 weight copies (HBM)", 0.0, (4.0 + 28.0 + 2.0 + 2.0) * eng.nflat)
    rows = {k: {"launches": round(v["launches"], 1), "gflop": round(v["flop"] / 1e9, 1), "mbytes": round(v["bytes"] / 1e6, 1),
                "mfma_ms": round(v["mfma_ms"], 3), "hbm_ms": round(v["hbm_ms"], 3), "floor_ms": round(v["floor_ms"], 3)}
            for k, v in fam.items()}
    tot = sum(v["floor_ms"] for v in fam.values())
    tot_m, tot_h = sum(v["mfma_ms"] for v in fam.values()), sum(v["hbm_ms"] for v in fam.values())
    return {"families": rows, "sum_floor_ms": round(tot, 3), "sum_mfma_ms": round(tot_m, 3), "sum_hbm_ms": round(tot_h, 3),
            "perfect_overlap_floor_ms": round(max(tot_m, tot_h), 3),
            "ms_per_step": round(ms_per_step, 3), "ms_per_step_over_sum_floor": round(ms_per_step / tot, 3),
            "mfma_peak_at_clock_tflops": at_clock_peak_tflops, "hbm_tbs": HBM_ACHIEVABLE_TBS,
            "note": "per launch max(algorithmic FLOP / at-clock MFMA peak, algorithmic bytes / 6.3 TB/s), summed without overlap; "
                    "perfect_overlap_floor_ms = max(all MFMA time, all HBM time): what two streams that never stall each other "
                    "could reach; the at-clock peak is 2.5 PFLOP/s x (clock held inside the GEMM main loops / 2.4 GHz), profiles/r06_clock.json"}


class _CachedEvents:
    """Event streams held in host memory (what a page-cached .npy folder is to the reference's loaders): built once in the
    parent, shared with the forked DataLoader workers.  source(i) -> (N,4) float64 ndarray."""

    def __init__(self, source, n):
        self.items = [source(i) for i in range(n)]

    def __call__(self, i):
        return self.items[i % len(self.items)]


def config5_figure(B=64, steps=5, warmup=2):
    """BASELINE configs[4] on ONE GPU: MEM pretrain ViT-Large/16 (D 1024, depth 24, 16 heads, layer scale 1e-5,
    mem/modeling_pretrain.py:22-140 with the reference's `pt_vit_large`-style arguments) on 480 x 640 2-bin voxels = 30 x 40 + 1
    = 1201 tokens (streaming attention, 4664-entry bias table), 600 masked patches per sample, bf16, stochastic depth 0.1,
    AdamW; a step = masks + forward + CE + backward + clip + AdamW on a batch resident in HBM.  B = 64 per GPU (the
    reference's global 512 over 8 GPUs; profiles/r04_vitl_batch.log: B 16: 222, B 32: 248, B 48: 259, B 64: 267 samples/s with the round-4 attention kernels,
    73.5 GB of the 288 GB).  FLOPs: 2 635.5 GFLOP per sample fwd + bwd (GEMMs only)."""
    import contextlib
    import io
    import numpy as np
    import torch
    from mem_amd import ops
    from mem_amd.masking_generator import MaskingGenerator
    from mem_amd.modeling_pretrain import pt_vit
    from mem_amd.optim_factory import FlatAdamW, get_parameter_groups
    H, W, FL = 480, 640, 2635.5e9
    torch.manual_seed(0)
    model = pt_vit(img_size=(H, W), patch_size=(16, 16), in_chans=2, vocab_size=8192, embed_dim=1024, depth=24, num_heads=16,
                   mlp_ratio=4, drop_path_rate=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False,
                   init_values=1e-5).cuda().train()
    eng = model.engine
    with contextlib.redirect_stdout(io.StringIO()):
        groups = get_parameter_groups(model, 0.05, model.no_weight_decay())
    opt = FlatAdamW(model, groups, lr=1e-4)
    opt.max_norm = 30.0
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand((B, 2, H, W), generator=g, device="cuda") * (torch.rand((B, 2, H, W), generator=g, device="cuda") < 0.3)
    masker = MaskingGenerator((30, 40), 600, min_num_patches=16, seed=1)
    pool = torch.randint(0, 8192, (B * 600,), device="cuda")

    def step():
        m = torch.from_numpy(masker.batch_u8(B).reshape(B, -1).astype(bool)).cuda()
        la = model.forward_loss(x, m, pool[: int(m.sum())])
        model.backward()
        eng.grad_norm()
        opt.step()
        return la
    for _ in range(warmup):
        la = step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    exec_fl = 0.0
    for _ in range(steps):
        la = step()
        exec_fl += executed_flop_per_sample(eng, 2)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    exec_fl /= steps
    # one instrumented step (HIP events around every GEMM product and attention launch, one stream): family shares
    ops.GEMM_EVENT_POOL = [torch.cuda.Event(enable_timing=True) for _ in range(2 * 700)]
    for e in ops.GEMM_EVENT_POOL:
        e.record()
    torch.cuda.synchronize()
    ops.GEMM_TIMER = log = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); step(); e1.record()
    torch.cuda.synchronize()
    ops.GEMM_TIMER = None
    inst_ms = e0.elapsed_time(e1)
    fam = {"nt_gemm": [0.0, 0.0], "weight_gradient_gemm": [0.0, 0.0], "attention_forward": [0.0, 0.0], "attention_backward": [0.0, 0.0]}
    for a0, a1, fl, code in log:
        k = ("attention_forward" if code == 200 else "attention_backward" if code == 201 else
             "weight_gradient_gemm" if 100 <= code <= 104 else "nt_gemm")
        fam[k][0] += a0.elapsed_time(a1); fam[k][1] += fl
    out = {"workload": "BASELINE configs[4], one GPU: MEM pretrain ViT-Large/16, 480x640 2-bin voxels (1201 tokens, 600 masked), bf16, "
                       f"batch {B}; step = masks + fwd/CE/bwd + clip + AdamW",
           "batch": B, "value": round(B / dt, 2), "unit": "samples/sec", "ms_per_step": round(dt * 1e3, 2), "steps": steps,
           "model_flops_frac_of_peak": round(B / dt * exec_fl / (PEAK_BF16_TFLOPS * 1e12), 4),
           "model_flops_frac_of_peak_reference_count": round(B / dt * FL / (PEAK_BF16_TFLOPS * 1e12), 4),
           "executed_flop_per_sample": round(exec_fl), "reference_flop_per_sample": FL,
           "last_loss": round(float(la[0].item()), 4), "max_mem_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1),
           "family_split_one_stream_step": {k: {"ms": round(v[0], 2), "share": round(v[0] / inst_ms, 3),
                                                "tflops": round(v[1] / (v[0] * 1e-3) / 1e12, 1) if v[0] else None}
                                            for k, v in fam.items()},
           "instrumented_step_ms": round(inst_ms, 2),
           "note": "family split: HIP events around every launch of one extra step run on ONE stream (the default step overlaps the "
                   "weight gradients with the dgrad chain on a second stream); rocprofv3 summary of the same workload: "
                   "profiles/r05_final_vitl_kernel_stats.csv (counters: r05_final_vitl_mfma_util.json, r05_final_vitl_traffic.json); "
                   "attention = the slot-layout kernels of csrc/attn_win.hip (round 5; attn_stream.hip: MEMHIP option attn_win = 0)"}
    del model, opt, eng, x
    torch.cuda.empty_cache()
    return out


def entrypoint_figure(model, opt, B, steps, warmup, workers, lr_sched):
    """The drop-in entrypoint as a user runs it (run_mem_pretraining.py:330-347,392-412): engine_for_pretraining.
    train_one_epoch over torch DataLoader(num_workers, pin_memory) of RawEventDataset -- N-Caltech101 geometry (240 x 180
    sensor, per-sample extents, data-dependent canvases), SliceRandomMaxEvs 30 000, the ncaltech.conf augmentation chain
    (random shift / flips, Resize(antialias), EventRandAugment, ColorJitter) batched on the GPU, the CLI's default tokenizer
    (fp16x2, CERTIFIED since round 5: labels equal to the fp32 mode's by construction, `with_tokenizer`) producing the labels, block-wise masks drawn per sample in the workers -- with the 246 MB of events of every batch
    crossing PCIe inside the timed region.  Returns samples/s over `steps` steps after `warmup`, and the stages timed alone."""
    import contextlib
    import io
    import numpy as np
    import torch
    from mem_amd import datasets as D, engine_for_pretraining as E
    from mem_amd.run_mem_pretraining import get_args
    from mem_amd.utils import NativeScalerWithGradNormCount
    from mem_amd.vae_model import DiscreteVAE, HipTokenizer
    dev = torch.device("cuda")
    with contextlib.redirect_stdout(io.StringIO()):
        args = get_args(["--expweek", "bench", "--data_path", "x/ncaltech101/", "--synthetic_if_missing", "1",
                         "--input_H", "224", "--input_W", "224", "--batch_size", str(B), "--num_mask_patches", "98",
                         "--normalize_events", "1", "--rand_aug", "1", "--color_jitter", "0.2", "--max_random_shift_evs", "8",
                         "--num_workers", str(workers), "--clip_grad", "30.0", "--synthetic_samples", str(B * (steps + warmup))])
        args.window_size = (14, 14)
        ds = D.build_pretraining_dataset(args)
        ds.source = _CachedEvents(ds.source, 512)
    with torch.random.fork_rng(devices=[]):          # the same random tokenizer weights in every run and figure (the share of
        torch.manual_seed(20251)                      # near-tie tokens, hence of certified recomputes, depends on them)
        vae = DiscreteVAE(input_H=224, input_W=224, num_tokens=8192, codebook_dim=512, num_layers=4, num_resnet_blocks=3,
                          hidden_dim=384, channels=3)
    vae = vae.cuda().eval()
    # the tokenizer the CLI builds by default (run_mem_pretraining.py: --tokenizer_impl: hip_fp16x2, certified)
    tok_prec = {"hip": "fp32", "hip_fp16x2": "fp16x2", "hip_bf16": "bf16"}[args.tokenizer_impl]
    tok = HipTokenizer(vae, max_batch=B, precision=tok_prec)
    loader = torch.utils.data.DataLoader(ds, batch_size=B, shuffle=False, num_workers=workers, pin_memory=bool(args.pin_mem),
                                         drop_last=True, collate_fn=ds.collate, prefetch_factor=2 if workers else None)
    marks = {}

    class Timed:
        def __len__(self):
            return len(loader)

        def __iter__(self):
            for i, b in enumerate(loader):
                if i == warmup:
                    torch.cuda.synchronize()
                    marks["t0"] = time.perf_counter()
                yield b
    scaler = NativeScalerWithGradNormCount()
    with contextlib.redirect_stdout(io.StringIO()):
        stats = E.train_one_epoch(model, tok, Timed(), opt, dev, 0, scaler, 30.0, lr_schedule_values=lr_sched,
                                  wd_schedule_values=None, args=args)
    torch.cuda.synchronize()
    dt = time.perf_counter() - marks["t0"]
    cert = tok.certification_stats() if hasattr(tok, "certification_stats") else None
    # the stages alone, on one batch (device time by events; H2D from the pinned batch the loader hands over)
    batch, _ = next(iter(torch.utils.data.DataLoader(ds, batch_size=B, shuffle=False, num_workers=0, pin_memory=True,
                                                     collate_fn=ds.collate)))

    def dev_ms(fn, n=3):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n
    ev_dev = batch["events"].to(dev, non_blocking=True)
    h2d = dev_ms(lambda: batch["events"].to(dev, non_blocking=True))
    aug = dev_ms(lambda: batch["pipe"](ev_dev, batch["offsets"], batch["draws"]))
    img = batch["pipe"](ev_dev, batch["offsets"], batch["draws"])
    tok_ms = dev_ms(lambda: tok.get_codebook_indices(img))
    t_host0 = time.perf_counter()
    for _ in range(3):
        batch["pipe"].pack(batch["draws"], batch["offsets"])
    pack_ms = (time.perf_counter() - t_host0) / 3 * 1e3
    del loader
    return {"value": round(B * steps / dt, 1), "unit": "samples/sec", "ms_per_step": round(dt / steps * 1e3, 2), "steps": steps,
            "warmup": warmup, "workers": workers, "pin_memory": bool(args.pin_mem), "batch": B,
            "events_bytes_per_step": int(batch["events"].numel() * 8), "last_loss": round(float(stats["loss"]), 4),
            "stages_alone_ms": {"h2d_events": round(h2d, 2), "augment_chain": round(aug, 2), "tokenizer_" + tok_prec: round(tok_ms, 2),
                                "host_pack_draws": round(pack_ms, 2)},
            "tokenizer_certification": (None if not cert else
                                        {"flagged_samples_per_batch": round(cert["flagged_samples"] / max(1, cert["calls"]), 1),
                                         "batches": cert["calls"], "kappa": cert["kappa"],
                                         "note": "samples recomputed on the fp32 kernels because a token's fp16x2 top-2 gap was within "
                                                 "kappa x the row rms (random tokenizer weights; sparse event images repeat near-ties)"}),
            "workload": "mem_amd.engine_for_pretraining.train_one_epoch over DataLoader(RawEventDataset): N-Caltech101 geometry "
                        "(data-dependent canvases), ncaltech.conf augmentations, " + tok_prec + " tokenizer labels (the CLI default), ViT-B/16 bf16, "
                        "events cross PCIe inside the timed region; event streams served from host memory"}


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or "unknown"


def _raster_worker(args):
    from oracle import events_np as E
    import numpy as np
    seed, n, reps = args
    g = np.random.default_rng(seed)
    ev = np.stack([g.integers(0, 224, n), g.integers(0, 224, n), np.sort(g.integers(0, 300000, n)),
                   g.integers(0, 2, n) * 2 - 1], 1).astype(np.float64)
    t0 = time.perf_counter()
    for _ in range(reps):
        E.event_arr_to_img(ev, 224, 224, False)
    return reps * n / (time.perf_counter() - t0)


def _mask_worker(args):
    import contextlib, io, random
    from oracle import masking_py as MP
    seed, reps = args
    random.seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        mg = MP.BlockMaskOracle((14, 14), 98, min_num_patches=16)
    t0 = time.perf_counter()
    for _ in range(reps):
        mg()
    return reps / (time.perf_counter() - t0)


def cpu_baseline(batch=8, budget_s=10.0, max_threads=32):
    """The oracle (CPU restatement of the reference, proven equal to it in the build container) timed on this box's host
    cores: fp32 eager PyTorch ViT-B fwd + CE + bwd + clip + AdamW at batch 8 (headline `value`)
    and batch 2 (BASELINE configs[0]), the np.add.at rasterizer and the pure-Python block-mask generator single-core and
    on all cores (process pool).  Bounded sample: ~10 s for the model leg, ~1 s per other leg.
    Thread count is capped for the model: eager CPU PyTorch at batch 8 gets slower, not faster, beyond a few dozen
    threads (256 threads measured 75 s/step on the GPU box)."""
    import torch
    from oracle import vit_ref as V
    from oracle.gen_golden import BASE, vit_inputs
    from mem_amd.utils import host_cpu_budget
    ncpu = host_cpu_budget()                          # the container's CPU quota, not the machine's core count
    threads = max(1, min(ncpu, max_threads))
    torch.set_num_threads(threads)
    cfg = dict(BASE, in_chans=2, drop_path_rate=0.0)
    m = V.RefViT(**cfg)
    opt = V.make_optimizer(m)

    def leg(b, budget):
        x, mask, labels = vit_inputs(cfg, b, 7, 98)
        V.train_step(m, opt, x, mask, labels, 0, clip_grad=30.0)            # warm-up
        t0 = time.time()
        steps = 0
        while steps < 1 or (time.time() - t0 < budget and steps < 50):
            V.train_step(m, opt, x, mask, labels, steps + 1, clip_grad=30.0)
            steps += 1
        dt = time.time() - t0
        return b * steps / dt, steps, dt
    v8, steps, dt = leg(batch, budget_s)
    v2, steps2, dt2 = leg(2, 3.0)
    out = {"value": round(v8, 3), "unit": "samples/sec", "cores": threads, "kind": "port", "cpu_model": _cpu_model(),
           "cores_on_box": ncpu, "cores_of_machine": os.cpu_count(),
           "sample": f"ViT-B/16 C=2 fp32 eager CPU (oracle/vit_ref.py), batch {batch}, {steps} steps "
                     f"after 1 warm-up in {dt:.1f} s, {threads} threads of the {ncpu} CPUs the container may use",
           "batch2": {"value": round(v2, 3), "unit": "samples/sec", "steps": steps2,
                      "sample": "BASELINE configs[0] shape: the same model at batch 2"}}
    try:
        import multiprocessing as mp
        nproc = max(1, min(ncpu, 64))
        r1 = _raster_worker((0, 30000, 20))
        k1 = _mask_worker((0, 2000))
        with mp.get_context("fork").Pool(nproc) as pool:
            rn = sum(pool.map(_raster_worker, [(i, 30000, 20) for i in range(nproc)]))
            kn = sum(pool.map(_mask_worker, [(i, 2000) for i in range(nproc)]))
        out["rasterizer"] = {"events_per_sec_1core": round(r1), "events_per_sec_all": round(rn), "processes": nproc,
                             "sample": "np.add.at rasterizer (oracle/events_np.py), 30 000 events on 224x224, 20 reps per process"}
        out["mask_generator"] = {"masks_per_sec_1core": round(k1), "masks_per_sec_all": round(kn), "processes": nproc,
                                 "sample": "pure-Python block-wise MaskingGenerator (oracle/masking_py.py), 14x14 / 98 / min 16"}
    except Exception as e:                                                    # the extra legs are optional
        out["legs_skipped"] = str(e)
    return out


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(a, argv):
    """`python bench.py --gpus N` from a bare shell: start one fresh rank process per GPU through torchrun as a child
    (this process has imported neither torch nor HIP), relay the children's output, print rank 0's JSON line LAST."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    env["MEMHIP_BENCH_CHILD"] = "1"
    port = int(os.environ.get("MASTER_PORT") or _free_port())
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + argv
    print("[bench] self-launch:", " ".join(cmd), file=sys.stderr, flush=True)
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=None, text=True)
    result = None
    for line in proc.stdout:
        line = line.rstrip("\n")
        if line.startswith("{") and '"metric"' in line:
            result = line
        elif line:
            print(line, file=sys.stderr, flush=True)
    rc = proc.wait()
    if result is not None:
        print(result, flush=True)
    sys.exit(rc if rc != 0 or result is not None else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100, help="timed steps (SURVEY 8d: 100 after 20 warm-up)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256, help="per-GPU batch (BASELINE config: 256)")
    ap.add_argument("--events", type=int, default=30000)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the run, replay the last timed step's batch once on the starting state and write what the step computed "
                         "(loss, gradient norm, samples of the weights, gradients, AdamW moments and input voxels) as "
                         "DIR/<name>.npy, float32")
    ap.add_argument("--full", action="store_true",
                    help="measure everything beside the headline too (the figures the --no-* switches below leave out, and for "
                         "N > 1 the steps without the gradient exchange); off: the headline only")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-gemm-timer", action="store_true")
    ap.add_argument("--no-tokenizer-figure", action="store_true",
                    help="skip the secondary figure that adds the frozen dVAE tokenizer forward (stock PyTorch-ROCm)")
    ap.add_argument("--no-raster-figure", action="store_true",
                    help="skip the secondary figure for BASELINE configs[3] (rasterizer at 1 M events per sample)")
    ap.add_argument("--wgrad-group", type=int, default=None,
                    help="A/B: engine.wgrad_group (0: every weight gradient its own launch, 1: proj + qkv of a block as one, 2: fc2 + fc1 too)")
    ap.add_argument("--no-side-stream", action="store_true",
                    help="A/B: keep the weight-gradient GEMMs on the main stream (engine.wgrad_side_stream = False)")
    ap.add_argument("--fwd-split", action="store_true",
                    help="A/B: forward as an uneven two-stream split of the batch (engine.fwd_two_streams = True)")
    ap.add_argument("--no-fwd-split", action="store_true", help="(default since round 2; kept for old command lines)")
    ap.add_argument("--bucket-dtype", choices=["fp32", "bf16"], default="fp32",
                    help="N > 1: wire format of the gradient buckets (fp32 = the reference's DDP exchange; bf16: half the bytes)")
    ap.add_argument("--reserve-cus", type=int, default=-1,
                    help="N > 1: CUs the persistent GEMM / attention grids leave to RCCL while gradient buckets are in flight "
                         "(-1 = 16 when more than one rank runs, 0 in a one-rank run; one-rank dry-run A/B: "
                         "profiles/r03_rccl_dryrun.json -- reserving 16 CUs costs <= 0.3 ms of a 39 ms step)")
    ap.add_argument("--hook-join", action="store_true",
                    help="A/B: the gradient-bucket hook runs on the main stream behind a per-layer join of the two streams (round 4)")
    ap.add_argument("--no-dp-skip", action="store_true",
                    help="stochastic depth by masking (every sample computed, dropped ones multiplied by zero) instead of "
                         "work skipping: A/B switch")
    ap.add_argument("--gelu-dg", type=int, default=None, choices=[0, 1],
                    help="A/B switch: 1 = fc1 keeps gelu'(h) as fp16 for the backward (MUL_AUX), 0 = it keeps h (DGELU); default: the engine's")
    ap.add_argument("--opt-overlap", action="store_true",
                    help="A/B: AdamW + bf16 cast + transposed copies per layer bucket on their own stream beside the next forward "
                         "(ViTEngine.overlap_optimizer; measured slower, off by default) instead of one block in front of it")
    ap.add_argument("--no-tail-rows", action="store_true",
                    help="A/B switch: the last block's MLP branch on every row instead of only the rows that reach the head")
    ap.add_argument("--no-entrypoint-figure", action="store_true",
                    help="skip the measurement of the real entrypoint loop (train_one_epoch over a DataLoader)")
    ap.add_argument("--entrypoint-workers", type=int, default=10, help="DataLoader workers of the entrypoint figure")
    ap.add_argument("--no-config5-figure", action="store_true", help="skip the ViT-L/16 480x640 single-GPU figure (BASELINE configs[4])")
    ap.add_argument("--config5-batch", type=int, default=64)
    ap.add_argument("--no-config4-figure", action="store_true",
                    help="skip the secondary figure for BASELINE configs[3] end to end (1 M events per sample feeding ViT-B)")
    ap.add_argument("--rendezvous-only", action="store_true",
                    help="launch plumbing check without a GPU (tests/test_bench_launch.py): start the ranks, form a gloo "
                         "group, all-reduce one number, print a stub JSON line; measures nothing")
    ap.add_argument("--opt", action="append", default=[], metavar="NAME=VALUE",
                    help="kernel-selection option for A/B runs (memhip_set_option), e.g. --opt gemm_stagger=0")
    a = ap.parse_args()
    if not a.full:
        # a plain run: set-up, warm-up, the timed steps, the outputs, the line -- nothing that takes steps or runs of its own
        a.no_cpu_baseline = a.no_gemm_timer = a.no_tokenizer_figure = a.no_raster_figure = True
        a.no_entrypoint_figure = a.no_config4_figure = a.no_config5_figure = True
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(a, sys.argv[1:])                  # never returns

    import numpy as np
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    if world != a.gpus:
        sys.exit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world} (launch with --nproc-per-node {a.gpus}, or unset "
                 "WORLD_SIZE and let bench.py start the ranks itself)")
    if a.rendezvous_only:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group("gloo")
        t = torch.tensor([float(rank + 1)])
        dist.all_reduce(t)
        dist.barrier()
        dist.destroy_process_group()
        if rank == 0:
            print(json.dumps({"metric": "rendezvous-only (no measurement)", "value": None, "n_gpus": world,
                              "rank_sum": float(t.item())}), flush=True)
        return
    torch.cuda.set_device(local_rank)
    if a.opt:
        from mem_amd import _lib
        for kv in a.opt:
            k, v = kv.split("=")
            _lib.set_option(k, int(v))
    # MEMHIP_BENCH_FORCE_DIST=1: run the RCCL path (process group, parameter broadcast, per-bucket async all-reduce hooked
    # into backward, join before the optimizer) in a ONE-rank group -- a single-GPU dry run of what N > 1 executes
    force_dist = world == 1 and os.environ.get("MEMHIP_BENCH_FORCE_DIST") == "1"
    if world > 1 or force_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl")

    from mem_amd import datasets as D, ops
    from mem_amd.masking_generator import MaskingGenerator
    from mem_amd.modeling_pretrain import pt_vit
    from mem_amd.optim_factory import FlatAdamW, get_parameter_groups
    from mem_amd.parallel import GradReducer
    from mem_amd.utils import cap_host_threads, cosine_scheduler

    # the launch thread must not be throttled: torch's default intra-op pool (one spinning thread per core of the machine)
    # exhausts the container's CPU quota (mem_amd/utils.py: cap_host_threads)
    host_threads = cap_host_threads(4)
    B, NE, H, W, C = a.batch, a.events, 224, 224, 2
    torch.manual_seed(1234 + rank)
    model = pt_vit(img_size=(H, W), patch_size=(16, 16), in_chans=C, vocab_size=8192, embed_dim=768, depth=12,
                   num_heads=12, mlp_ratio=4, drop_path_rate=0.1, use_shared_rel_pos_bias=True,
                   use_abs_pos_emb=False, init_values=0.1).cuda().train()
    eng = model.engine
    eng.wgrad_side_stream = not a.no_side_stream
    if a.wgrad_group is not None:
        eng.wgrad_group = a.wgrad_group
    eng.dp_skip = not a.no_dp_skip
    if a.gelu_dg is not None:
        eng.set_gelu_dg(bool(a.gelu_dg))
    eng.tail_rows = not a.no_tail_rows
    eng.hook_on_side = not a.hook_join
    eng.overlap_optimizer = bool(a.opt_overlap)
    eng.fwd_two_streams = bool(a.fwd_split) and not a.no_fwd_split
    import contextlib, io
    with contextlib.redirect_stdout(io.StringIO()):
        groups = get_parameter_groups(model, 0.05, model.no_weight_decay())
        lr_sched = cosine_scheduler(5e-4, 1e-5, 3000, 1000, warmup_epochs=5, warmup_steps=1000)
    opt = FlatAdamW(model, groups, lr=5e-4)
    opt.max_norm = 30.0
    reducer = None
    if world > 1 or force_dist:
        if a.reserve_cus < 0:
            a.reserve_cus = 0          # (no A/B on more than one GPU exists: --reserve-cus 16 is the experiment, not the default)
        reducer = GradReducer(eng.flat_g, eng.buckets, flat_p=eng.flat_p, force=force_dist,
                              bucket_dtype=torch.bfloat16 if a.bucket_dtype == "bf16" else None, reserve_cus=a.reserve_cus,
                              streams=lambda: [torch.cuda.current_stream(), eng._side])
        eng.grad_hook = reducer
        eng.weights_dirty = True

    # ---- synthetic batch, resident in HBM (SURVEY.md section 8d recipe)
    g = np.random.default_rng(1234 + rank)
    ev = np.empty((B * NE, 4), dtype=np.float64)
    ev[:, 0] = g.integers(0, W, B * NE)
    ev[:, 1] = g.integers(0, H, B * NE)
    ev[:, 2] = np.sort(g.integers(0, 300000, (B, NE)), axis=1).reshape(-1)
    ev[:, 3] = g.integers(0, 2, B * NE) * 2 - 1
    ev_dev = torch.from_numpy(ev).cuda()
    offsets = (torch.arange(B + 1, dtype=torch.int64) * NE).cuda()
    pipe = D.EventBatchPipeline(H, W, out_chans=C, time_surface=False, train_augs=False)
    masker = MaskingGenerator((14, 14), 98, min_num_patches=16, seed=1234 + rank)
    label_pool = torch.randint(0, 8192, (B * 98,), generator=torch.Generator().manual_seed(1234 + rank)).cuda()
    T = eng.T
    from mem_amd.utils import HostStager
    st_rows, st_mask = HostStager(B * 98 * 4, "cuda"), HostStager(B * 196, "cuda")
    last_timed = a.warmup + a.steps - 1
    last_batch = {}                                                   # --dump-outputs: the batch of the last timed step

    def step(it, replay=None):
        for grp in opt.param_groups:
            grp["lr"] = lr_sched[it]
        x = pipe(ev_dev, offsets) if replay is None else replay["x"]   # rasterize + event_norm (HIP)
        m = masker.batch_u8(B).reshape(B, -1) if replay is None else replay["m"]   # host MT19937 (bit-exact CPython stream)
        if a.dump_outputs and replay is None and it == last_timed:
            dps = getattr(model, "_dp_stream", None)
            last_batch.update(x=x, m=m, dp=dps.state() if dps is not None and dps.gen is not None else None)
        bi, pi = np.nonzero(m)
        rows = st_rows.put((bi * T + 1 + pi).astype(np.int32))        # pinned ring: the host never waits for the queue
        mask_u8 = st_mask.put(m.reshape(-1))
        labels = label_pool[: rows.numel()]
        la = model.forward_loss(x, None, labels, rows=rows, mask_u8=mask_u8)
        model.backward()
        if reducer is not None:
            reducer.finish()
        eng.grad_norm()
        opt.step()
        return la

    def fence():
        torch.cuda.synchronize()
        if world > 1 or force_dist:
            dist.barrier()
            torch.cuda.synchronize()

    def replay_last_step():
        """--dump-outputs, after everything timed: the training step of the timed path, run once more on the batch of the last
        timed step (its voxels, masks, labels, stochastic-depth draws and learning rate) from the state the run started from.
        The fp32 gradient reductions of the step use atomics, so two runs differ in the last bits of a step, and training
        compounds that over the steps before the last; one step from the starting state is the same in every run up to
        rounding, and is what two builds are compared on.  Every rank runs it (the gradient exchange is collective)."""
        fence()
        eng.flat_p.copy_(start_p)
        eng.flat_g.zero_()
        opt.exp_avg.zero_()
        opt.exp_avg_sq.zero_()
        opt.steps = 0
        eng.weights_dirty = True                                    # the bf16 copies are cast again from the restored weights
        if last_batch["dp"] is None:
            model._dp_stream = None                                  # drawn from a fresh stream, as the first step did
        else:
            model._dp_stream.load_state(last_batch["dp"])
        la_r = step(last_timed, replay=last_batch)
        fence()
        if rank != 0:
            return None
        return dump_outputs(a.dump_outputs, {
            "loss_acc": la_r, "grad_norm": eng.gnorm, "weights": eng.flat_p[: eng.nflat], "grads": eng.flat_g[: eng.nflat],
            "adamw_exp_avg": opt.exp_avg, "adamw_exp_avg_sq": opt.exp_avg_sq, "voxels": last_batch["x"]})

    # --dump-outputs: the state the run starts from (weights; AdamW moments and step count are zero), to replay the last
    # timed step's batch on after the run -- see replay_last_step
    start_p = eng.flat_p.clone() if a.dump_outputs else None
    for it in range(a.warmup):
        step(it)
    # CPython's cyclic collector walks every tracked object of the process (model, optimizer, torch internals) when its
    # allocation counters trip: ~14 ms of host stall every few steps, which the GPU sees as an idle gap because the
    # host runs only a few ms ahead.  Freeze what exists now into the permanent generation (gc stays enabled).
    import gc
    gc.collect()
    gc.freeze()
    fence()
    # Live per-launch GEMM timing (HIP events on the launch stream) for the roofline object.  Two event
    # records around each of the 149 GEMM products of a step cost ~1.2 ms of dispatch bubbles per step
    # (measured) and serialise the side stream, so few timed steps are instrumented (timer_steps).
    timer_log = [] if not a.no_gemm_timer else None
    timer_marks = []                                  # (first, last + 1) entries of timer_log per instrumented step
    if timer_log is not None:
        # pre-create and pre-record the timer's events (2 per GEMM product, ~150 products per instrumented step)
        need = 2 * 160 * (len(timer_steps(a.steps)) + POST_REGION_TIMER_STEPS)
        ops.GEMM_EVENT_POOL = [torch.cuda.Event(enable_timing=True) for _ in range(need)]
        for e in ops.GEMM_EVENT_POOL:
            e.record()
        torch.cuda.synchronize()
    # per-step durations for the median: one event per step boundary on the launch stream, read after the timed region
    step_ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    t0 = time.perf_counter()
    step_ev[0].record()
    host_t = [time.perf_counter()]
    inst = timer_steps(a.steps)
    exec_flop = 0.0
    for it in range(a.steps):
        ops.GEMM_TIMER = timer_log if (timer_log is not None and it in inst) else None
        i0 = len(timer_log) if timer_log is not None else 0
        la = step(a.warmup + it)
        step_ev[it + 1].record()
        host_t.append(time.perf_counter())
        exec_flop += executed_flop_per_sample(eng, C)
        if ops.GEMM_TIMER is not None:
            timer_marks.append((i0, len(timer_log)))
    exec_flop /= max(1, a.steps)                                    # mean executed GEMM FLOPs per sample of the timed steps
    ops.GEMM_TIMER = timer_log
    fence()
    dt = time.perf_counter() - t0
    # ---- more instrumented steps right BEHIND the timed region (round 6: one instrumented step inside K = 20 timed steps gave a
    # dominant-kernel figure that moved by 7 % between runs; every instrumented step costs ~5 ms, so the others do not sit
    # inside the region `value` is computed from).  The roofline pools all of them and lists the per-step figures.
    if timer_log is not None:
        for j in range(POST_REGION_TIMER_STEPS):
            i0 = len(timer_log)
            step(a.warmup + a.steps + j)
            timer_marks.append((i0, len(timer_log)))
        fence()
    if os.environ.get("MEMHIP_BENCH_STEP_TIMES") == "1":
        print("[bench] host per-step ms:", [round((host_t[i + 1] - host_t[i]) * 1e3, 1) for i in range(a.steps)], file=sys.stderr)
        print("[bench] per-step ms:", [round(step_ev[i].elapsed_time(step_ev[i + 1]), 2) for i in range(a.steps)], file=sys.stderr)
    step_ms = sorted(step_ev[i].elapsed_time(step_ev[i + 1]) for i in range(a.steps))
    # un-instrumented steps only: the GEMM event pairs of an instrumented step cost ~1.2 ms
    plain = sorted(step_ev[i].elapsed_time(step_ev[i + 1]) for i in range(a.steps) if timer_log is None or i not in inst)
    timer, ops.GEMM_TIMER = ops.GEMM_TIMER, None
    loss_last = float(la[0].item())
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    # ---- N > 1 (and the one-rank RCCL dry run): what RCCL saw, and how much of the gradient exchange is EXPOSED -- the
    # same ranks run the same steps once more with the exchange switched off (no collective is issued; backward, norm and
    # AdamW unchanged); per-step times by HIP events, median per rank, MAX over ranks
    rccl_info = None
    if reducer is not None and a.full:
        ranks = [None] * dist.get_world_size()
        prop = torch.cuda.get_device_properties(torch.cuda.current_device())
        dist.all_gather_object(ranks, {"rank": dist.get_rank(), "local_rank": local_rank, "device_index": torch.cuda.current_device(),
                                       "device": prop.name, "gcn_arch": getattr(prop, "gcnArchName", None),
                                       "pci_bus_id": getattr(prop, "pci_bus_id", None), "host": os.uname().nodename})
        n_ref = min(10, a.steps)
        reducer.active = False
        fence()
        # (the no-exchange reference keeps the CU reservation: what it isolates is the exchange, not the smaller grids)
        if reducer.reserve_cus > 0:
            reducer._reserve(True)
        ref_ev = [torch.cuda.Event(enable_timing=True) for _ in range(n_ref + 1)]
        ref_ev[0].record()
        for it in range(n_ref):
            step(a.warmup + a.steps + it)
            ref_ev[it + 1].record()
        fence()
        reducer.release()
        reducer.active = True
        ref_ms = sorted(ref_ev[i].elapsed_time(ref_ev[i + 1]) for i in range(n_ref))
        # ... and once more with NO bucket hook at all (= the single-GPU headline path on this rank): what the data-parallel
        # plumbing itself costs (stream waits of the hook, the join before the norm)
        hook, eng.grad_hook = eng.grad_hook, None
        nh_ev = [torch.cuda.Event(enable_timing=True) for _ in range(n_ref + 1)]
        nh_ev[0].record()
        for it in range(n_ref):
            step(a.warmup + a.steps + n_ref + it)
            nh_ev[it + 1].record()
        fence()
        eng.grad_hook = hook
        nh_ms = sorted(nh_ev[i].elapsed_time(nh_ev[i + 1]) for i in range(n_ref))
        med = torch.tensor([plain[len(plain) // 2] if plain else step_ms[len(step_ms) // 2], ref_ms[len(ref_ms) // 2],
                            nh_ms[len(nh_ms) // 2]], dtype=torch.float64, device="cuda")
        dist.all_reduce(med, op=dist.ReduceOp.MAX)
        with_x, without_x, no_hook = float(med[0].item()), float(med[1].item()), float(med[2].item())
        rccl_info = {"world_size": dist.get_world_size(), "backend": dist.get_backend(), "ranks": ranks,
                     "distinct_pci_bus_ids": len({str(r.get("pci_bus_id")) for r in ranks if r}),     # = world_size on a real N-GPU run
                     "buckets_per_step": len(eng.buckets), "bytes_per_step": reducer.bytes_per_step,
                     "bucket_dtype": a.bucket_dtype, "reserve_cus": a.reserve_cus,
                     "ms_per_step_p50_with_exchange": round(with_x, 3), "ms_per_step_p50_without_exchange": round(without_x, 3),
                     "allreduce_exposed_ms": round(with_x - without_x, 3),
                     "ms_per_step_p50_no_hook": round(no_hook, 3), "exchange_minus_no_hook_ms": round(with_x - no_hook, 3),
                     "hook_stream": "side (main stream never joins per layer)" if eng.hook_on_side else "main (per-layer join)",
                     "note": "exchange = one asynchronous all-reduce per gradient bucket, issued from backward's bucket hook, "
                             "joined before the gradient norm; `without` = the same steps on the same ranks with no collective "
                             "issued (medians of per-step HIP-event times, MAX over ranks)"}

    # ---- secondary figure: the frozen tokenizer forward that the reference runs every step to make the
    # labels (engine_for_pretraining.py:144); not part of `value` (BASELINE: tokenizer outside the timed set)
    tok_ms = tok_bf16_ms = tok_torch_ms = tok_step_ms = tok_f16x2_ms = tok_f16x2_step_ms = tok_label_stat = None
    if not a.no_tokenizer_figure and world == 1:                      # N=1 figures only: ranks must reach the teardown together
        try:
            from mem_amd.vae_model import DiscreteVAE, HipTokenizer
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(20251)
                vae = DiscreteVAE(input_H=H, input_W=W, num_tokens=8192, codebook_dim=512, num_layers=4,
                                  num_resnet_blocks=3, hidden_dim=384, channels=3)
            vae = vae.cuda().eval()
            img = torch.rand(B, 3, H, W, device="cuda")

            def _time(fn, n):
                for _ in range(2):
                    fn()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(n):
                    fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t1) / n * 1e3
            tok = HipTokenizer(vae, max_batch=B)                       # default mode: fp32 operands, exact labels
            tok_ms = _time(lambda: tok.get_codebook_indices(img), 3)
            # label exactness of the split-precision mode, measured here (not assumed): fp32 ids and their top-2 logit gaps
            # on two batches of RASTERISED synthetic streams (positive / time-surface / negative planes, the second batch
            # mirrored in x) and on the uniform-random batch that is timed: 3 x B x 196 tokens >= 1.5e5
            from mem_amd import datasets as D2
            raster = D2.rasterize(ev_dev, offsets, H, W, True, strict=False).float() / 255.0
            ev_m = ev_dev.clone(); ev_m[:, 0] = (W - 1) - ev_m[:, 0]
            raster_m = D2.rasterize(ev_m, offsets, H, W, True, strict=False).float() / 255.0
            del ev_m
            label_sets = {"rasterised": raster, "rasterised_mirrored": raster_m, "uniform_random": img}
            ids32, gap32 = {}, {}
            for name, im in label_sets.items():
                ids32[name] = tok.get_codebook_indices(im).clone()
                gap32[name] = tok.last_top2_gap(im.shape[0]).clone()
            # the REAL combined step, as engine_for_pretraining runs it: tokenizer on its own stream beside the ViT trunk,
            # its ids (gathered at the masked positions) are the labels the loss waits for
            side_t = torch.cuda.Stream()
            st_flat = HostStager(B * 98 * 8, "cuda")

            def combined_ms(tk, n_tok_steps=6):
                def step_tok(it):
                    for grp in opt.param_groups:
                        grp["lr"] = lr_sched[it]
                    x = pipe(ev_dev, offsets)
                    m = masker.batch_u8(B).reshape(B, -1)
                    bi, pi = np.nonzero(m)
                    rows = st_rows.put((bi * T + 1 + pi).astype(np.int32))
                    flat = st_flat.put((bi * 196 + pi).astype(np.int64))
                    mask_u8 = st_mask.put(m.reshape(-1))
                    e0 = torch.cuda.Event(); e0.record()
                    with torch.cuda.stream(side_t):
                        side_t.wait_event(e0)
                        labels = tk.get_codebook_indices(img).reshape(-1).index_select(0, flat)
                        e1 = torch.cuda.Event(); e1.record(side_t)
                    labels.record_stream(torch.cuda.current_stream())     # allocated on the side stream, consumed on the main one
                    model.forward_loss(x, None, labels, rows=rows, mask_u8=mask_u8, labels_event=e1)
                    model.backward()
                    eng.grad_norm()
                    opt.step()
                for it in range(2):
                    step_tok(it)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for it in range(n_tok_steps):
                    step_tok(2 + it)
                torch.cuda.synchronize()
                return (time.perf_counter() - t1) / n_tok_steps * 1e3
            tok_step_ms = combined_ms(tok)
            del tok
            # raw split-precision forward (no certification) beside the certified default: what the margins + the fp32
            # recompute of the flagged samples cost
            tok = HipTokenizer(vae, max_batch=B, precision="fp16x2", certify=False)
            tok_f16x2_raw_ms = _time(lambda: tok.get_codebook_indices(img), 5)
            raw_bad = sum(int((tok.get_codebook_indices(im) != ids32[name]).sum()) for name, im in label_sets.items())
            del tok
            tok = HipTokenizer(vae, max_batch=B, precision="fp16x2")
            tok_f16x2_ms = _time(lambda: tok.get_codebook_indices(img), 5)
            tok_f16x2_step_ms = combined_ms(tok)
            cert0 = tok.certification_stats()
            n_tok = n_bad = 0
            bad_gaps, min_gap = [], float("inf")
            for name, im in label_sets.items():
                ids16 = tok.get_codebook_indices(im)
                bad = ids16 != ids32[name]
                n_tok += ids16.numel(); n_bad += int(bad.sum())
                if bool(bad.any()):
                    bad_gaps += gap32[name][bad].tolist()
                min_gap = min(min_gap, float(gap32[name].min()))
            tok_label_stat = {"tokens_compared": n_tok, "label_mismatches": n_bad,
                              "label_mismatch_per_million": round(n_bad / n_tok * 1e6, 2),
                              "fp32_top2_gap_at_mismatches_max": (max(bad_gaps) if bad_gaps else None),
                              "fp32_top2_gap_min_over_all_tokens": min_gap,
                              "certified": True, "raw_fp16x2_label_mismatches": raw_bad,
                              "raw_fp16x2_tokenizer_ms": round(tok_f16x2_raw_ms, 3),
                              "certification": (lambda c1: {"kappa": c1["kappa"], "exact_capacity": c1["exact_capacity"],
                                                            "flagged_samples_in_label_sets": c1["flagged_samples"] - cert0["flagged_samples"],
                                                            "samples_in_label_sets": 3 * B})(tok.certification_stats()),
                              "inputs": "2 x %d rasterised synthetic event streams (3 planes, the second mirrored) + %d uniform-random "
                                        "images, 196 tokens each; ids of the fp32 mode are the reference (equal to the reference "
                                        "tokenizer's on the committed fixtures, tests/test_tokenizer_gpu.py)" % (B, B)}
            del raster, raster_m, label_sets, ids32, gap32
            del tok
            tok = HipTokenizer(vae, max_batch=B, precision="bf16")
            tok_bf16_ms = _time(lambda: tok.get_codebook_indices(img), 5)
            tok_torch_ms = _time(lambda: vae.get_codebook_indices(img), 2)
            del vae, img, tok
        except Exception as e:                                        # the figure is optional
            print(f"[bench] tokenizer figure skipped: {e}", file=sys.stderr)
    # ---- secondary figure: the REAL entrypoint loop (DataLoader workers, H2D, augmentation chain, tokenizer, ViT)
    entry_fig = None
    if world == 1 and not a.no_entrypoint_figure:
        try:
            entry_fig = entrypoint_figure(model, opt, B, 20, 4, a.entrypoint_workers, lr_sched)
        except Exception as e:                                        # the figure is optional
            import traceback
            traceback.print_exc()
            print(f"[bench] entrypoint figure skipped: {e}", file=sys.stderr)
    # ---- secondary figure: BASELINE configs[3], the rasterizer alone at N-ImageNet scale (1 M events per
    # sample, 480 x 640 canvas): HBM-bound, algorithmic bytes = 32 B per event + 3*H*W output bytes
    raster_fig = None
    if world == 1 and not a.no_raster_figure:
        try:
            from mem_amd import datasets as D
            rb, rn, rh, rw = 32, 1_000_000, 480, 640
            g = torch.Generator(device="cuda").manual_seed(4)
            ev = torch.stack([torch.randint(0, rw, (rb * rn,), generator=g, device="cuda").double(),
                              torch.randint(0, rh, (rb * rn,), generator=g, device="cuda").double(),
                              torch.rand((rb * rn,), generator=g, device="cuda", dtype=torch.float64) * 3e5,
                              (torch.randint(0, 2, (rb * rn,), generator=g, device="cuda") * 2 - 1).double()], 1).contiguous()
            off = torch.arange(0, rb + 1, device="cuda", dtype=torch.int64) * rn
            for _ in range(2):
                D.rasterize(ev, off, rh, rw, False, strict=False)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                D.rasterize(ev, off, rh, rw, False, strict=False)
            e1.record()
            torch.cuda.synchronize()
            rdt = e0.elapsed_time(e1) * 1e-3 / 10
            byts = rb * (32 * rn + 3 * rh * rw)
            raster_fig = {"workload": "BASELINE configs[3]: rasterizer, 1 M events per sample (f64 (N,4) rows), 480x640 canvas, "
                                      "32 samples per launch", "events_per_sec": round(rb * rn / rdt),
                          "us_per_sample": round(rdt / rb * 1e6, 2),
                          "roofline": {"bound": "hbm", "kernel": "raster_bin_keys + raster_bin_accum",
                                       "achieved": round(byts / rdt / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
                                       "frac": round(byts / rdt / 8e12, 4), "algorithmic_bytes_per_sample": 32 * rn + 3 * rh * rw,
                                       "traffic": None}}
            # the same kernels at 64 samples per launch (what profiles/r06_final_raster_* trace): launch gaps and the last, partly
            # filled round of pass-2 workgroups weigh half as much
            try:
                ev = torch.cat([ev, ev]); off = torch.arange(0, 2 * rb + 1, device="cuda", dtype=torch.int64) * rn
                for _ in range(2):
                    D.rasterize(ev, off, rh, rw, False, strict=False)
                e0.record()
                for _ in range(10):
                    D.rasterize(ev, off, rh, rw, False, strict=False)
                e1.record()
                torch.cuda.synchronize()
                raster_fig["frac_at_64_samples_per_launch"] = round(2 * byts / (e0.elapsed_time(e1) * 1e-3 / 10) / 8e12, 4)
            except Exception as e2:
                print(f"[bench] rasterizer 64-sample figure skipped: {e2}", file=sys.stderr)
            # HBM bytes per launch from the PMC passes (tools/prof_pmc_raster.sh -> profiles/raster_traffic.json)
            per_sample = raster_traffic_per_sample()
            if per_sample is not None:
                raster_fig["roofline"]["traffic"] = round(per_sample * rb)
        except Exception as e:                                        # the figure is optional
            print(f"[bench] rasterizer figure skipped: {e}", file=sys.stderr)
        finally:
            ev = off = None                                          # 1 GB of events: released on every path
            torch.cuda.empty_cache()
    # ---- secondary figure: BASELINE configs[3] END TO END -- N-ImageNet-scale streams (1 M events per sample on the
    # 640 x 480 sensor) feeding the same ViT-B step.  Policy (stated): the reference's N-ImageNet evaluation chain,
    # ReshapeScaleXandY(newH = newW = 224, oldH = 480, oldW = 640, is_train = False) (mem/datasets.py:464-485,615-621:
    # x *= 224/640, y *= 224/480 in float64) fused into the rasterizer's single read of the events, EventArrToImg on the
    # 224 x 224 canvas, then the benchmark's event transforms, masks and training step unchanged.  No SliceRandomMaxEvs:
    # the whole 1 M-event stream is binned (the reference caps a sample at < 200 000 events).
    cfg4 = None
    if world == 1 and not a.no_config4_figure:
        try:
            n4 = 1_000_000
            g4 = torch.Generator(device="cuda").manual_seed(44)
            ev4 = torch.stack([torch.randint(0, 640, (B * n4,), generator=g4, device="cuda").double(),
                               torch.randint(0, 480, (B * n4,), generator=g4, device="cuda").double(),
                               torch.rand((B * n4,), generator=g4, device="cuda", dtype=torch.float64) * 3e5,
                               (torch.randint(0, 2, (B * n4,), generator=g4, device="cuda") * 2 - 1).double()], 1).contiguous()
            off4 = torch.arange(0, B + 1, device="cuda", dtype=torch.int64) * n4
            aug4 = D._new_aug_array(B)
            aug4["scale_x"], aug4["scale_y"] = 224 / 640, 224 / 480
            aug4_dev = torch.from_numpy(aug4.view(np.uint8).reshape(-1).copy()).cuda()
            from mem_amd import transforms as T4

            def step4(it):
                for grp in opt.param_groups:
                    grp["lr"] = lr_sched[it]
                img = D.rasterize(ev4, off4, H, W, False, aug4_dev, strict=False)
                x = T4.event_norm(img, pipe.flags, pipe.num_stds, 0.5, C)
                m = masker.batch_u8(B).reshape(B, -1)
                bi, pi = np.nonzero(m)
                rows = st_rows.put((bi * T + 1 + pi).astype(np.int32))
                mask_u8 = st_mask.put(m.reshape(-1))
                la = model.forward_loss(x, None, label_pool[: rows.numel()], rows=rows, mask_u8=mask_u8)
                model.backward()
                eng.grad_norm()
                opt.step()
                return la
            for it in range(2):
                step4(it)
            # median of seven steps, each between its own pair of events (all seven are in the line): as a five-step mean this
            # figure came out at 35.8 or at 40.1 ms from one run of bench.py to the next on one box, with the round-5 library as
            # with this one (cause not isolated: something in one step, not in the kernels -- the rasterizer and the ViT step
            # timed alone do not move)
            n_it = 7
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(n_it + 1)]
            e1, e2 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            marks[0].record()
            for it in range(n_it):
                step4(2 + it)
                marks[it + 1].record()
            e1.record()
            for _ in range(n_it):
                D.rasterize(ev4, off4, H, W, False, aug4_dev, strict=False)
            e2.record()
            torch.cuda.synchronize()
            per_step = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(n_it))
            ms4 = per_step[n_it // 2]
            msr = e1.elapsed_time(e2) / n_it
            byts = B * (32 * n4 + 3 * H * W)
            cfg4 = {"workload": "BASELINE configs[3] end to end: 1 M events per sample (640x480 sensor, f64 (N,4) rows) -> "
                                "ReshapeScaleXandY to 224x224 fused into the rasterizer -> event_norm -> masks -> ViT-B/16 "
                                f"fwd/CE/bwd + clip + AdamW, batch {B}",
                    "value": round(B / (ms4 * 1e-3), 1), "unit": "samples/sec", "ms_per_step": round(ms4, 3),
                    "events_per_sec": round(B * n4 / (ms4 * 1e-3)),
                    "ms_per_step_all": [round(v, 2) for v in per_step], "estimator": "median of 7 steps",
                    "rasterizer_ms_per_step": round(msr, 3),
                    "rasterizer_roofline": {"bound": "hbm", "achieved": round(byts / (msr * 1e-3) / 1e9, 1), "peak": 8000.0,
                                            "unit": "GB/s", "frac": round(byts / (msr * 1e-3) / 8e12, 4),
                                            "algorithmic_bytes_per_sample": 32 * n4 + 3 * H * W}}
            del ev4
        except Exception as e:                                        # the figure is optional
            print(f"[bench] config #4 figure skipped: {e}", file=sys.stderr)
    cfg5 = None
    if world == 1 and not a.no_config5_figure:
        try:
            cfg5 = config5_figure(a.config5_batch)
        except Exception as e:                                        # the figure is optional
            import traceback
            traceback.print_exc()
            print(f"[bench] config #5 figure skipped: {e}", file=sys.stderr)
    dumped = replay_last_step() if a.dump_outputs else None
    if rank == 0:
        ms = dt / a.steps * 1e3
        value = world * B * a.steps / dt
        roof = sol = None
        if timer:
            n_inst = len(timer_marks)
            tot_ms, tot_fl, per = 0.0, 0.0, {}
            attn_per = {}
            for e0, e1, fl, epi in timer:
                d = e0.elapsed_time(e1)
                if int(epi) >= 200:                                   # fused attention launches (ops._timed): own family
                    k = attn_per.setdefault(int(epi), [0, 0.0, 0.0])
                    k[0] += 1; k[1] += d; k[2] += fl
                    continue
                tot_ms += d
                tot_fl += fl
                k = per.setdefault(int(epi), [0, 0.0, 0.0])
                k[0] += 1; k[1] += d; k[2] += fl
            ach = tot_fl / (tot_ms * 1e-3) / 1e12
            # HBM bytes per launch from the PMC passes (tools/prof_pmc.sh -> profiles/gemm_traffic.json;
            # FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for gfx950), None until collected
            tj = _load_profile("gemm_traffic.json") or {}
            fam = {str(k): {"launches": v[0], "avg_us": round(v[1] / v[0] * 1e3, 2),
                            "tflops": round(v[2] / (v[1] * 1e-3) / 1e12, 1)} for k, v in sorted(per.items())}
            # the dominant kernel of the step is the weight-gradient GEMM (tn_p8_body of gemm_tn_p8.hip, launched product by
            # product as gemm_tn_p8_kernel -- logged as 100 -- or as a group of n products in one grid, gemm_tn_p8_group_kernel,
            # logged as 100 + n); launches / avg_launch_us count PRODUCTS (a pair = 2)
            dom = None
            for code, n_prod in ((100, 1), (102, 2), (103, 3), (104, 4)):
                if code in per:
                    v = per[code]
                    dom = [v[0] * n_prod, v[1], v[2]] if dom is None else [dom[0] + v[0] * n_prod, dom[1] + v[1], dom[2] + v[2]]
            # the same figure per instrumented step (how far one step's sample is from the pooled mean).  A step whose figure sits
            # more than 10 % below the MEDIAN of the instrumented steps was disturbed from outside (seen once in ~40 instrumented
            # steps on this pool: every weight-gradient product of one step 40 % slower, the steps before and behind it normal):
            # it is listed (`disturbed_steps`) and left out of achieved / frac / avg_launch_us, which pool the others; the figure
            # over ALL steps is `frac_all_steps`
            per_step_frac, per_step_dom = [], []
            for i0, i1 in timer_marks:
                fl_s = ms_s = 0.0
                n_s = 0
                for e0, e1, fl, epi in timer[i0:i1]:
                    if int(epi) in (100, 102, 103, 104):
                        fl_s += fl; ms_s += e0.elapsed_time(e1); n_s += max(1, int(epi) - 100)
                if ms_s > 0:
                    per_step_frac.append(round(fl_s / (ms_s * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4))
                    per_step_dom.append((n_s, ms_s, fl_s))
            disturbed, frac_all, n_dom_steps = [], None, n_inst
            if dom and len(per_step_frac) >= 3:
                med = sorted(per_step_frac)[len(per_step_frac) // 2]
                keep = [i for i, f in enumerate(per_step_frac) if f >= 0.9 * med]
                disturbed = [{"step": i, "frac": per_step_frac[i]} for i in range(len(per_step_frac)) if i not in keep]
                if disturbed and keep:
                    frac_all = round(dom[2] / (dom[1] * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4)
                    dom = [sum(per_step_dom[i][0] for i in keep), sum(per_step_dom[i][1] for i in keep), sum(per_step_dom[i][2] for i in keep)]
                    n_dom_steps = len(keep)
            if dom:
                d_ach = dom[2] / (dom[1] * 1e-3) / 1e12
                roof = {"bound": "mfma", "kernel": "gemm_tn_p8_kernel / gemm_tn_p8_group_kernel (bf16 weight-gradient GEMM, split over token rows)",
                        "achieved": round(d_ach, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(d_ach / PEAK_BF16_TFLOPS, 4),
                        "traffic": wgrad_traffic_per_product(tj),
                        "launches": dom[0], "avg_launch_us": round(dom[1] / dom[0] * 1e3, 2),
                        "algorithmic_flop_per_launch": round(dom[2] / dom[0]),
                        "share_of_step": round(dom[1] / (dt * 1e3 * n_dom_steps / a.steps), 3),
                        "instrumented_steps": n_inst, "instrumented_steps_inside_timed_region": len(inst),
                        "frac_per_instrumented_step": per_step_frac, "disturbed_steps": disturbed, "frac_all_steps": frac_all,
                        "kernel_vs_reduction": wgrad_kernel_split(),
                        "products_in_group_launches": sum(per[c][0] * (c - 100) for c in (102, 103, 104) if c in per),
                        "note": "HIP events around one weight-gradient call = gemm_tn_p8_kernel + its tn_reduce_kernel, or the group "
                                "kernel (proj + qkv of a block in one grid) + its reduction pass; launches / avg_launch_us are per PRODUCT; the "
                                "instrumented steps run on ONE stream (the events serialise the side stream), so compare with the "
                                "sequential rocprofv3 summary (profiles/r06_final_seq_kernel_stats.csv; the steady-state steps alone: r06_final_seq_step_kernels.txt), not with the "
                                "two-stream one, where concurrent launches stretch every kernel.  achieved / frac / avg_launch_us pool "
                                "every instrumented step: the one(s) inside the timed region and POST_REGION_TIMER_STEPS more run right "
                                "behind it (an instrumented step costs ~5 ms, so they are kept out of `value`); frac_per_instrumented_step "
                                "lists them one by one; kernel_vs_reduction splits a product into the GEMM kernel and its reduction pass "
                                "from the committed rocprofv3 summary (the events bracket both)"}
            else:
                roof = {"bound": "mfma", "kernel": "bf16 MFMA GEMM family", "achieved": round(ach, 1),
                        "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / PEAK_BF16_TFLOPS, 4),
                        "traffic": None}
            # MFMA-pipe utilisation from the SQ counters (tools/prof_mfma.sh -> profiles/mfma_util.json, own PMC passes):
            # SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE x 1024 SIMDs), per kernel family and over the whole step
            util = mfma_util_by_kernel()
            if util is not None:
                roof["mfma_util_pmc"] = util
            # the clock the chip holds inside the GEMM main loops (a committed measurement, not this run's), and what the
            # achieved rate is against the peak AT THAT CLOCK next to the 2.5 PFLOP/s spec peak
            clk = kernel_clock()
            if clk is not None:
                clk["frac_of_at_clock_peak"] = round(roof["achieved"] / clk["at_clock_peak_tflops"], 4)
                roof["clock"] = clk
            try:
                sol = speed_of_light(eng, (H, W), NE, clk["at_clock_peak_tflops"] if clk else PEAK_BF16_TFLOPS, ms)
            except Exception as e:                                    # a reporting object must never cost the headline
                print(f"[bench] speed_of_light skipped: {e!r}", file=sys.stderr)
            # the honest headline next to the dominant kernel: the model-level rate of the WHOLE step (all kernels, all
            # gaps) against the dense bf16 peak, and the GEMM family as a whole (below)
            ws = value / world * exec_flop / 1e12
            ws_ref = value / world * FLOP_PER_SAMPLE[C] / 1e12
            roof["whole_step"] = {"achieved": round(ws, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                                  "frac": round(ws / PEAK_BF16_TFLOPS, 4),
                                  "executed_flop_per_sample": round(exec_flop),
                                  "reference_flop_per_sample": FLOP_PER_SAMPLE[C],
                                  "frac_on_reference_flop_count": round(ws_ref / PEAK_BF16_TFLOPS, 4),
                                  "ms_per_step": round(ms, 3)}
            if eng.dp_skip:
                # the reference computes every sample of every block and multiplies the dropped ones by zero
                # (modeling_finetune.py:42-53); the work-skipping engine does not launch them: say how much that is
                rates = [float(b.drop_prob) for b in model.blocks]
                roof["whole_step"]["block_flops_not_executed_frac"] = round(sum(rates) / max(1, len(rates)), 4)
            if eng.tail_rows and eng.cur.get("tail") is not None:
                # dead-row elimination: the last block's MLP branch (2 GEMMs of D x 4D, fwd + dgrad + wgrad) runs on the
                # rows that reach the head only (Mm of M token rows)
                t_, d_, hd_ = eng.T, eng.D, eng.hidden
                mlp_frac = 3.0 * 2.0 * 2.0 * t_ * d_ * hd_ / FLOP_PER_SAMPLE[C]
                roof["whole_step"]["last_block_mlp_flops_not_executed_frac"] = round(
                    mlp_frac * (1.0 - eng.cur["Mm"] / float(eng.cur["M"])), 4)
            roof["whole_step"]["note"] = ("achieved / frac count the GEMM FLOPs the engine EXECUTED (mean over the timed steps: kept "
                                          "samples per stochastic-depth branch, masked rows in the last block's MLP); "
                                          "frac_on_reference_flop_count prices the same step time with the reference's count "
                                          "(every sample in every branch, BASELINE.md section 2) -- A/B with --no-dp-skip --no-tail-rows")
            if attn_per:
                roof["attention_family"] = {("forward" if k == 200 else "backward"): {
                    "launches": v[0], "avg_us": round(v[1] / v[0] * 1e3, 2), "tflops": round(v[2] / (v[1] * 1e-3) / 1e12, 1),
                    "share_of_step": round(v[1] / (dt * 1e3 * n_inst / a.steps), 3)} for k, v in sorted(attn_per.items())}
            roof["gemm_family"] = {"kernels": "gemm_p8_kernel<EPI>, gemm_nt_kernel<EPI>, gemm_tn_p8_kernel",
                                   "achieved": round(ach, 1), "frac": round(ach / PEAK_BF16_TFLOPS, 4),
                                   "launches": len(timer), "avg_launch_us": round(tot_ms / len(timer) * 1e3, 2),
                                   "share_of_step": round(tot_ms / (dt * 1e3 * n_inst / a.steps), 3), "per_epilogue": fam,
                                   "traffic": {k: v.get("hbm_bytes_per_launch") for k, v in tj.items() if k.startswith("gemm")}}
        from mem_amd import _lib as _L
        out = {"metric": "pretrain samples/sec (ViT-B, 224^2 event voxels)", "value": round(value, 1),
               "unit": "samples/sec", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
               "ms_per_step": round(ms, 3), "ms_per_step_p50": round(step_ms[len(step_ms) // 2], 3),
               "ms_per_step_p50_uninstrumented": round(plain[len(plain) // 2], 3) if plain else None,
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": "bf16", "data": "synthetic", "full": a.full,
               "config": {"workload": "MEM pretrain ViT-Base/16, 224^2 2-bin event voxels, bf16, batch 256 per GPU "
                                      "(BASELINE configs[1]); step = rasterize 256x30k events + event_norm + masks "
                                      "+ ViT fwd/CE/bwd + clip + AdamW",
                          "global_batch": world * B, "events_per_sample": NE, "parallelism": f"dp{world}",
                          "model_flops_frac_of_peak": round(value / world * exec_flop / (PEAK_BF16_TFLOPS * 1e12), 4),
                          "model_flops_frac_of_peak_reference_count": round(value / world * FLOP_PER_SAMPLE[C] / (PEAK_BF16_TFLOPS * 1e12), 4),
                          "last_loss": round(loss_last, 4), "host_threads": host_threads,
                          "stochastic_depth": "work skipping" if eng.dp_skip else "masked",
                          "optimizer": ("AdamW + bf16 cast + transposed copies per layer bucket on their own stream, the next forward waits "
                                        "per bucket" if eng.overlap_optimizer else "AdamW as one launch in front of the next forward"),
                          "last_block_mlp_rows": "rows that reach the head" if eng.tail_rows else "all"},
               "roofline": roof}
        if roof is not None and sol is not None:
            out["speed_of_light"] = sol
        out["library"] = {"path": os.path.relpath(_L.LIB_PATH, ROOT), "build_flags": _L.BUILD_FLAGS, "shipped_build": _L.IS_SHIPPED_LIB,
                          "abi": _L.ABI_VERSION, "options_set": sorted(a.opt)}
        if dumped is not None:
            out["outputs"] = {"dir": a.dump_outputs, "arrays": dumped,
                              "step": "the last timed step's batch, replayed once on the starting state after the run",
                              "note": "float32 .npy; [shape written, elements of the array]: an array of more than "
                                      f"{DUMP_SAMPLE} elements is a fixed, seeded sample of them"}
        if not _L.IS_SHIPPED_LIB:
            # a measurement build (MEMHIP_LIB / extra compiler flags) is never the headline: the A/B tools read ab_value
            out["metric"] = "NOT THE HEADLINE: measurement build of libmemhip.so (MEMHIP_LIB / build flags set) -- " + out["metric"]
            out["ab_value"], out["value"] = out["value"], None
        if tok_ms is not None:
            fp32_fig = {"value": round(world * B / (tok_step_ms * 1e-3), 1), "unit": "samples/sec",
                        "ms_per_step": round(tok_step_ms, 3), "sequential_sum_ms": round(ms + tok_ms, 3),
                        "tokenizer_ms_per_step": round(tok_ms, 3),
                        "tokenizer_tflops": round(B * 24.4e9 / (tok_ms * 1e-3) / 1e12, 1), "tokenizer_fp32_peak_tflops": 157.3,
                        "note": "--tokenizer_impl hip: fp32 operands and accumulation like the reference (csrc/conv_f32.hip, "
                                "v_mfma_f32_16x16x4_f32)"}
            f16_fig = None if tok_f16x2_ms is None else {
                "value": round(world * B / (tok_f16x2_step_ms * 1e-3), 1), "unit": "samples/sec",
                "ms_per_step": round(tok_f16x2_step_ms, 3), "tokenizer_ms_per_step": round(tok_f16x2_ms, 3),
                **(tok_label_stat or {}),
                "note": "--tokenizer_impl hip_fp16x2 (the entrypoint's default): two fp16 planes per value, three fp16 MFMAs per "
                        "product; CERTIFIED (round 5): a label is kept only where its top-2 gap exceeds kappa x the row rms, every "
                        "sample holding a token below that margin is recomputed on the fp32 kernels on the device (no host sync) "
                        "-- labels equal the fp32 mode's by construction; `raw_fp16x2_tokenizer_ms` is the forward without that step"}
            # the primary figure is the mode the entrypoint runs by default -- the split-precision one, PROVIDED it reproduced
            # every label of the fp32 mode on the tokens compared in this very run; otherwise the fp32 mode
            exact = bool(f16_fig) and bool(tok_label_stat) and tok_label_stat["label_mismatches"] == 0
            prim = f16_fig if exact else fp32_fig
            out["with_tokenizer"] = {"value": prim["value"], "unit": "samples/sec", "ms_per_step": prim["ms_per_step"],
                                     "mode": "hip_fp16x2" if exact else "hip (fp32)",
                                     "label_mismatch_per_million_vs_fp32_mode": (tok_label_stat or {}).get("label_mismatch_per_million"),
                                     "fp16x2_mode": f16_fig, "fp32_mode": fp32_fig,
                                     "tokenizer_ms_bf16_mode": round(tok_bf16_ms, 3) if tok_bf16_ms else None,
                                     "tokenizer_ms_stock_torch_fp32": round(tok_torch_ms, 3) if tok_torch_ms else None,
                                     "note": "secondary figure (SURVEY section 8d): the same step WITH the frozen dVAE "
                                             "tokenizer forward producing the labels, MEASURED as the training loop runs it "
                                             "(tokenizer on its own HIP stream beside the ViT trunk; the loss waits for its "
                                             "ids); tokenizer forward (4 conv + 3 ResBlocks + 1x1 -> 8192, 24.4 GFLOP/sample, "
                                             "random weights).  value = the entrypoint's default tokenizer mode (certified fp16x2: labels equal to "
                                             "the fp32 mode's by construction, and compared with them on every token of this run), else "
                                             "the fp32 mode; the opt-in "
                                             "bf16-operand mode (csrc/conv.hip, 1-3 % of labels differ) and the fp32 torch module "
                                             "on stock PyTorch-ROCm are timed beside it"}
        if rccl_info is not None:
            out["rccl"] = rccl_info
        if entry_fig is not None:
            out["entrypoint"] = entry_fig
            if tok_ms is not None:
                out["entrypoint"]["vs_with_tokenizer"] = round(entry_fig["value"] / out["with_tokenizer"]["value"], 3)
        if raster_fig is not None:
            out["rasterizer_1m_events"] = raster_fig
        if cfg4 is not None:
            out["config4_end_to_end"] = cfg4
        if cfg5 is not None:
            out["config5_vitl_1gpu"] = cfg5
        if world == 1 and not a.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline()
        result_line = json.dumps(out)
    else:
        result_line = None
    if world > 1 or force_dist:
        dist.destroy_process_group()
    # RCCL prints its version banner through C stdio (buffered until exit when stdout is a pipe): flush it first so that
    # the JSON line is the LAST line on stdout
    import ctypes
    try:
        ctypes.CDLL(None).fflush(None)
    except OSError:
        pass
    if result_line is not None:
        print(result_line, flush=True)


if __name__ == "__main__":
    main()
