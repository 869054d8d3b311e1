"""-m gpu: data-parallel FINETUNING (stage 3).  Two real rank processes (tests/ft_ddp_worker.py) on the one GPU of the test box --
gloo on CUDA tensors, because RCCL refuses two ranks per device -- run the product's attach helper and the product's loop
(engine_for_finetuning.train_one_epoch) on ft_vit in the FT_A geometry (64 x 96 image, D = 128, depth 3, T = 25): 4 samples per
rank, 3 optimizer steps, plain CE, clip 1.0, layer decay 0.75, the ranks starting from DIFFERENT weights.  One pair of processes
runs the five variants in turn (plain, update_freq 2, drop path 0.2 + dropout 0.1 with per-rank streams, frozen backbone, EMA).

Every variant: the two ranks' flat_p are bit-identical (without the broadcast and the exchange they are not: the ranks start
from different weights and see different shards).  EMA: the twins are bit-identical too.  Frozen: the trunk range of flat_p is
what rank 0 broadcast, and one bucket is exchanged per step.  plain / update_freq 2 against ONE rank running the same loop on the
concatenated batches (global batch 8): per-rank mean CE over equal per-rank batches makes the mean of the ranks' gradients the
global gradient, so the runs differ by bf16 accumulation order only (a split batch changes which rows share a tile and the
order of fp32 atomics) -- the bars are those of the pretraining twin of this comparison (tests/test_ddp_gpu.py): mean loss
within 2e-3, relative difference of the 3-step parameter update within 2e-2.  The loss is plain CE taken in fp32 on the model's
bf16 logits (ft_ddp_worker.plain_ce: what the reference computes under autocast); nn.CrossEntropyLoss() on the bf16 logits
returns a bf16 loss in steps of 2^-6, too coarse for the bar -- the first run measured |d| = 2.604e-3 = 2^-6 / 6 with it.
Measured on one MI355X: plain |d loss| 1.5e-6, update 1.4e-3; update_freq 2 |d loss| 1.8e-6, update 1.7e-3.

Last, one process: the entrypoint's main() on synthetic data with no process group behaves as before (same log.txt keys, no
reducer attached)."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

LOSS_TOL, PARAM_REL_TOL = 2e-3, 2e-2
RANK_TIME_LIMIT = 300                      # seconds, each rank process
_FAULT = []                                # a rank process that died or ran out of time: nothing more is started here


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ft_ddp_worker as W
    return W


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    """{variant: (record of rank 0, record of rank 1)} from ONE pair of rank processes."""
    tmp = tmp_path_factory.mktemp("ft_ddp")
    port = _free_port()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    outs = [str(tmp / f"rank{r}.pt") for r in range(2)]
    logs = [open(tmp / f"rank{r}.log", "w") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "ft_ddp_worker.py"), "--rank", str(r), "--world", "2",
                               "--port", str(port), "--out", outs[r]], env=env, stdout=logs[r], stderr=subprocess.STDOUT)
             for r in range(2)]
    codes = []
    for p in procs:
        try:
            codes.append(p.wait(timeout=RANK_TIME_LIMIT))
        except subprocess.TimeoutExpired:
            codes.append("time limit")
    for p in procs:
        if p.poll() is None:
            p.kill()
            p.wait(30)
    for f in logs:
        f.close()
    if codes != [0, 0]:
        _FAULT.append(codes)
        tails = "\n".join(open(tmp / f"rank{r}.log").read()[-3000:] for r in range(2))
        pytest.fail(f"rank processes ended with {codes}\n{tails}")
    r0, r1 = torch.load(outs[0]), torch.load(outs[1])
    return {v: (r0[v], r1[v]) for v in r0}


_SINGLE = {}


def _single(variant):
    """The one-rank job of the same loop on the concatenated batches, once per variant."""
    if _FAULT:
        pytest.fail(f"a rank process failed before ({_FAULT[0]}): nothing more is started on the GPU")
    if variant not in _SINGLE:
        _SINGLE[variant] = _worker().run_variant(variant, 2, None)
    return _SINGLE[variant]


@pytest.mark.parametrize("variant", ["plain", "accum", "drop", "frozen", "ema"])
def test_two_ranks_hold_identical_parameters(ranks, variant):
    r0, r1 = ranks[variant]
    assert r0["opt_steps"] == r1["opt_steps"] == 3
    assert torch.equal(r0["flat_p0"], r1["flat_p0"]), "the broadcast did not give every rank rank 0's weights"
    assert not torch.equal(r0["flat_p"], r0["flat_p0"]), "nothing was trained"
    assert torch.equal(r0["flat_p"], r1["flat_p"]), "ranks diverged: the gradient exchange did not keep the replicas equal"
    assert r0["pending"] == r1["pending"] == 0                      # the loop released the reducer
    assert r0["calls"] == r1["calls"]                               # the same buckets in the same order on every rank
    if variant != "frozen":
        # every bucket once per UPDATE step (update_freq 2: 6 micro-steps, still 3 exchanges), none twice
        n = r0["n_buckets"]
        assert len(r0["calls"]) == 3 * n and all(sorted(r0["calls"][i * n:(i + 1) * n]) == list(range(n)) for i in range(3))
    print("%s: %d buckets, %d bytes per update step, calls %s" % (variant, len(r0["last_exchanged"]), r0["bytes_per_step"],
                                                                   r0["calls"][:r0["n_buckets"]]))


def test_two_ranks_hold_identical_ema(ranks):
    r0, r1 = ranks["ema"]
    assert torch.equal(r0["ema_flat_p"], r1["ema_flat_p"]), "rank-local EMA updates of identical parameters diverged"
    assert not torch.equal(r0["ema_flat_p"], r0["flat_p"]) and not torch.equal(r0["ema_flat_p"], r0["flat_p0"])


def test_frozen_trunk_exchanges_the_head_bucket_only(ranks):
    r0, r1 = ranks["frozen"]
    he = r0["head_end"]
    for r in (r0, r1):
        assert torch.equal(r["flat_p"][he:], r["flat_p0"][he:]), "a frozen run changed the trunk range of flat_p"
        assert not torch.equal(r["flat_p"][:he], r["flat_p0"][:he])
        assert r["calls"] == [0, 0, 0] and r["last_exchanged"] == [0]          # one bucket per step: the head
        assert r["bytes_per_step"] == 4 * he


@pytest.mark.parametrize("variant", ["plain", "accum"])
def test_two_ranks_match_one_rank_on_the_concatenated_batches(ranks, variant):
    r0, r1 = ranks[variant]
    one = _single(variant)
    assert torch.equal(one["flat_p0"], r0["flat_p0"])               # the one-rank job starts from rank 0's weights
    dloss = abs(one["loss"] - r0["loss"])
    upd = (one["flat_p"] - one["flat_p0"]).norm()
    rel = float((r0["flat_p"] - one["flat_p"]).norm() / upd)
    print("%s: mean loss 1 rank %.6f, 2 ranks %.6f (|d| = %.3e, bar %.0e); relative difference of the 3-step parameter update "
          "%.3e (bar %.0e); grad norm %.5f vs %.5f" % (variant, one["loss"], r0["loss"], dloss, LOSS_TOL, rel, PARAM_REL_TOL,
                                                       one["grad_norm"], r0["grad_norm"]))
    assert r0["loss"] == r1["loss"]                                 # the meters are averaged over the ranks
    assert dloss <= LOSS_TOL
    assert rel <= PARAM_REL_TOL


LOG_KEYS = {"train_lr", "train_min_lr", "train_loss", "train_class_acc", "train_loss_scale", "train_weight_decay",
            "train_grad_norm", "test_loss", "test_acc1", "test_acc5", "ema_test_loss", "ema_test_acc1", "ema_test_acc5", "epoch",
            "n_parameters"}


def test_entrypoint_without_a_process_group_behaves_as_before(tmp_path, monkeypatch):
    if _FAULT:
        pytest.fail(f"a rank process failed before ({_FAULT[0]}): nothing more is started on the GPU")
    from mem_amd import run_class_finetuning as RC
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SLURM_PROCID"):
        monkeypatch.delenv(k, raising=False)
    seen = []
    get_model = RC.get_model
    monkeypatch.setattr(RC, "get_model", lambda a: seen.append(get_model(a)) or seen[-1])
    threads = torch.get_num_threads()
    args = RC.get_args(["--expweek", "t", "--data_path", "synthetic", "--nb_classes", "4", "--input_H", "64", "--input_W", "96",
                        "--batch_size", "8", "--synthetic_samples", "16", "--num_workers", "0", "--transformer_depth", "2",
                        "--transformer_emb", "128", "--transformer_heads", "2", "--rand_aug", "0", "--slice_max_evs", "5000",
                        "--output_dir", str(tmp_path), "--layer_decay", "0.75", "--lr", "1e-3", "--epochs", "1",
                        "--warmup_epochs", "0", "--model_ema_decay", "0.9"])
    try:
        RC.main(args)
    finally:
        torch.set_num_threads(threads)
    assert args.distributed is False and len(seen) == 1
    m = seen[0]
    assert m.engine.grad_hook is None and getattr(m, "_reducer", None) is None
    log = [json.loads(line) for line in open(tmp_path / "log.txt")]
    assert len(log) == 1 and set(log[0]) == LOG_KEYS, sorted(set(log[0]) ^ LOG_KEYS)
    ck = torch.load(tmp_path / "checkpoint-0.pth", map_location="cpu", weights_only=False)
    assert ck["numerics"]["precision"] == "bf16" and ck["drop_path_rng"]["world"] == 1 and "model_ema" in ck
