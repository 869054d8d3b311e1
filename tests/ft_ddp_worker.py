"""One data-parallel rank of the tiny FINETUNING job used by tests/test_ft_ddp_gpu.py (run as a subprocess), and the same job on
one rank (imported by the test): ft_vit in the FT_A geometry, the product's attach helper (parallel.attach_reducer with the
StepExchange the finetuning entrypoint uses: parameter broadcast from rank 0 BEFORE the EMA twin and the optimizer exist, gradient
buckets from the engine's backward hook) and the product's loop (engine_for_finetuning.train_one_epoch) on this rank's slice of a
fixed global batch.  Backend gloo on CUDA tensors: both ranks share the ONE GPU of the test box (RCCL refuses two ranks on one
device); the collective's arithmetic (SUM, then / world) is the same.  One process runs every variant in turn (one start-up for
all of them):

    plain | accum (update_freq 2) | drop (drop path 0.2, dropout 0.1, per-rank streams) | frozen (freeze_backbone) | ema

Mirrors the reference's mem/run_class_finetuning.py (DistributedSampler split, DDP after :559) and mem/engine_for_finetuning.py:113-130."""
import argparse
import contextlib
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

VARIANTS = ("plain", "accum", "drop", "frozen", "ema")
STEPS, PER_RANK, SEED_W, LR, CLIP, LAYER_DECAY = 3, 4, 3, 1e-3, 1.0, 0.75


class _Counting:
    """Between the StepExchange and its GradReducer: the bucket index of every collective started."""

    def __init__(self, reducer):
        self._r, self.calls = reducer, []

    def __call__(self, k):
        self.calls.append(k)
        self._r(k)

    def __getattr__(self, name):
        return getattr(self._r, name)


def plain_ce():
    """Plain cross-entropy taken in fp32 on the model's bf16 logits -- what the reference's loop computes (autocast runs
    cross_entropy in fp32) and what engine_for_finetuning.evaluate does.  nn.CrossEntropyLoss() on the bf16 logits themselves
    returns a bf16 loss: steps of 2^-6 = 1.6e-2 at a loss of 2.4, which cannot resolve the 2e-3 bar of the comparison (the
    first run of this test measured |d| = 2.604e-3 = exactly one such step on one of six per-rank losses, 2^-6 / 6)."""
    import torch

    class PlainCE(torch.nn.Module):
        def forward(self, logits, target):
            return torch.nn.functional.cross_entropy(logits.float(), target)
    return PlainCE()


def batches(world, rank, variant):
    """This rank's micro-batches (rank=None: the concatenated global batches of the one-rank job), on the host."""
    import torch
    from oracle.gen_golden_ft import FT_A, ft_inputs
    out = []
    for it in range(STEPS * (2 if variant == "accum" else 1)):
        parts = [ft_inputs(FT_A, PER_RANK, 5000 + 10 * it + r) for r in range(world)]
        out.append(parts[rank] if rank is not None else (torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])))
    return out


def run_variant(variant, world, rank):
    """Model, attach (rank is not None), EMA, optimizer, one epoch of the product loop; returns the record the test compares."""
    import torch
    from oracle.gen_golden_ft import FT_A
    from oracle.vit_ref import fill_by_name
    from mem_amd import engine_for_finetuning as EF
    from mem_amd import optim_factory as OF
    from mem_amd import utils as U
    from mem_amd.modeling_finetune import ft_vit
    from mem_amd.parallel import attach_reducer
    cfg = dict(FT_A, **(dict(drop_path_rate=0.2, drop_rate=0.1) if variant == "drop" else {}))
    m = ft_vit(**cfg)
    # every rank starts from DIFFERENT weights except rank 0 / the one-rank job: the broadcast must fix that
    m.load_state_dict(fill_by_name(m.state_dict(), seed=SEED_W + (rank or 0)))
    if variant == "frozen":
        m.freeze_backbone()
    m = m.cuda().train()
    eng = m.engine
    m._dp_stream = U.DropPathStream()
    m._dp_stream.seed(11 + (rank or 0))                            # per-rank drop-path / dropout streams, as the entrypoint seeds them
    gate = None
    if rank is not None:
        gate = attach_reducer(m, eng, step_exchange=True)
        gate.reducer = _Counting(gate.reducer)
    p0 = eng.flat_p.clone()
    ema = U.ModelEma(m, decay=0.9) if variant == "ema" else None
    depth = m.get_num_layers()
    assigner = OF.LayerDecayValueAssigner([LAYER_DECAY ** (depth + 1 - i) for i in range(depth + 2)])

    class OA:
        opt = "adamw"; weight_decay = 0.05; opt_eps = 1e-8; lr = LR
    with contextlib.redirect_stdout(io.StringIO()):
        opt = OF.create_optimizer(OA(), m, skip_list=m.no_weight_decay(), get_num_layer=assigner.get_layer_id,
                                  get_layer_scale=assigner.get_scale)
        stats = EF.train_one_epoch(None, m, plain_ce(), batches(world, rank, variant), opt, torch.device("cuda"),
                                   0, U.NativeScalerWithGradNormCount(), max_norm=CLIP, model_ema=ema,
                                   update_freq=2 if variant == "accum" else 1)
    torch.cuda.synchronize()
    rec = {"flat_p": eng.flat_p.cpu(), "flat_p0": p0.cpu(), "loss": float(stats["loss"]), "grad_norm": float(stats["grad_norm"]),
           "head_end": int(eng.head_end), "opt_steps": int(opt.steps)}
    if ema is not None:
        rec["ema_flat_p"] = ema.ema.engine.flat_p.cpu()
    if gate is not None:
        rec.update(calls=list(gate.reducer.calls), last_exchanged=list(gate.last_exchanged), n_buckets=len(eng.buckets),
                   bytes_per_step=int(gate.bytes_per_step), pending=len(gate.reducer.handles))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int); ap.add_argument("--world", type=int); ap.add_argument("--port", type=int)
    ap.add_argument("--variants", default=",".join(VARIANTS)); ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port), RANK=str(a.rank), WORLD_SIZE=str(a.world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=a.rank, world_size=a.world)
    out = {}
    for v in a.variants.split(","):
        out[v] = run_variant(v, a.world, a.rank)
        print("rank %d: variant %s done, mean loss %.6f" % (a.rank, v, out[v]["loss"]), flush=True)
    torch.save(out, a.out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
