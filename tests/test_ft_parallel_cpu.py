"""-m "not gpu": the data-parallel finetuning loop on two gloo ranks with CPU tensors -- parallel.StepExchange (the gate
between the engine's gradient hook and GradReducer) alone on a stub flat buffer, and engine_for_finetuning.train_one_epoch
driving it with a toy model that keeps the engine's contract: parameters and their .grad are views of flat_p / flat_g, the
trunk's bucket is handed from inside backward, the head's gradients come from torch autograd alone.

  * accumulation (update_freq 2): hook calls of the first micro-step start no collective; after the second one every rank's
    flat_g is the mean over the ranks of the ACCUMULATED buffers, bit-identical between the ranks;
  * buckets the engine did not hand are handed once, in index order; a frozen trunk exchanges bucket 0 and nothing else;
  * a NaN loss on rank 1 in iteration 2 ends BOTH ranks with status 1 in that iteration (joined with a time limit: a rank
    left waiting in a collective fails here);
  * evaluate's averages over unequal shards are count-weighted."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

N_HEAD, N = 1024, 4 * 1024
BUCKETS = [("head", 0, N_HEAD), ("block1", N_HEAD, 2048), ("block0", 2048, 3072), ("embed", 3072, N)]


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _run_world2(worker, *extra, expect_exit=0, timeout=120):
    """Two spawned ranks; returns what they put on the queue, sorted by rank.  Every process is joined with a time limit and
    killed if it is still there afterwards (a blocked rank is a failure of the test, not a hang of the suite)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=worker, args=(r, 2, port, q) + extra) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted(q.get(timeout=timeout) for _ in procs)
        for p in procs:
            p.join(60)
        assert [p.exitcode for p in procs] == [expect_exit] * 2, [p.exitcode for p in procs]
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join(10)
    return res


def _grad(rank, micro):
    return torch.randn(N, generator=torch.Generator().manual_seed(1000 + 10 * rank + micro))


class _Spy:
    """Stands between a StepExchange and its GradReducer: logs (tag of the moment, bucket index) of every collective started."""

    def __init__(self, reducer, log, tag):
        self._r, self._log, self._tag = reducer, log, tag

    def __call__(self, k):
        self._log.append((self._tag(), k))
        self._r(k)

    def __getattr__(self, name):
        return getattr(self._r, name)


# ---------------------------------------------------------------------------------------------- the helper on a stub buffer
def _worker_gate(rank, world, port, q):
    _init(rank, world, port)
    from mem_amd.parallel import GradReducer, StepExchange
    flat_g = torch.zeros(N)
    gate = StepExchange(GradReducer(flat_g, BUCKETS))
    log, micro = [], [0]
    gate.reducer = _Spy(gate.reducer, log, lambda: micro[0])
    ok = gate.expected == [0, 1, 2, 3] and gate.bytes_per_step == 4 * N
    # ---- update_freq = 2: the stub engine adds its micro-batch gradient and hands every bucket, on both micro-steps
    for micro[0], do_update in ((1, False), (2, True)):
        gate.begin_micro_step(do_update)
        flat_g += _grad(rank, micro[0])
        for k in range(len(BUCKETS)):
            gate(k)
        if micro[0] == 1:
            ok = ok and log == [] and gate.reducer.handles == [] and gate.handed == []     # no collective was started
            ok = ok and torch.equal(flat_g, _grad(rank, 1))
    gate.finish()
    acc = [_grad(r, 1) + _grad(r, 2) for r in range(world)]
    ok = ok and torch.equal(flat_g, (acc[0] + acc[1]) / 2)         # gloo: SUM, then / world -- the mean of the ACCUMULATED buffers
    ok = ok and log == [(2, k) for k in range(4)] and gate.last_exchanged == [0, 1, 2, 3]
    both = [torch.empty(N), torch.empty(N)]
    dist.all_gather(both, flat_g)
    ok = ok and torch.equal(both[0], both[1])
    # ---- hand-over: the engine hands 2 then 1; finish() adds 0 and 3, once, in index order
    del log[:]
    micro[0] = 3
    gate.begin_micro_step(True)
    flat_g.copy_(_grad(rank, 3))
    gate(2); gate(1)
    missing = gate.hand_missing()
    ok = ok and missing == [0, 3] and gate.hand_missing() == []
    gate.finish()
    ok = ok and [k for _, k in log] == [2, 1, 0, 3]
    ok = ok and torch.equal(flat_g, (_grad(0, 3) + _grad(1, 3)) / 2)
    try:
        gate.begin_micro_step(True)
        gate(1); gate(1)
        ok = False
    except RuntimeError:
        gate.finish()                                              # (both ranks started bucket 1 once: join it)
    # ---- frozen: the stub engine hands nothing; bucket 0 alone is exchanged, the rest of the buffer is not touched
    del log[:]
    gate.set_frozen(True)
    ok = ok and gate.expected == [0] and gate.bytes_per_step == 4 * N_HEAD
    gate.begin_micro_step(True)
    flat_g.copy_(_grad(rank, 4))
    gate.finish()
    want = _grad(rank, 4)
    want[:N_HEAD] = ((_grad(0, 4) + _grad(1, 4)) / 2)[:N_HEAD]
    ok = ok and [k for _, k in log] == [0] and gate.last_exchanged == [0] and torch.equal(flat_g, want)
    gate(0)
    gate.release()
    ok = ok and gate.reducer.handles == [] and gate.handed == []
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


def test_step_exchange_gate_and_hand_over_world2():
    assert _run_world2(_worker_gate) == [(0, True), (1, True)]


def test_step_exchange_single_process_is_a_noop():
    from mem_amd.parallel import GradReducer, StepExchange, any_rank
    g = torch.ones(N)
    gate = StepExchange(GradReducer(g, BUCKETS), frozen=True)
    gate.begin_micro_step(True)
    gate.finish()
    assert torch.equal(g, torch.ones(N)) and gate.last_exchanged == [0]
    assert any_rank(None, True) and not any_rank(None, False) and any_rank(gate, True) and not any_rank(gate, False)


# ---------------------------------------------------------------------------------------------- the product loop, toy model
D, V = 8, 4


class _ToyEngine:
    def __init__(self):
        n_head, n = 1024, 2048                                      # head bucket [0, 1024), trunk bucket [1024, 2048)
        self.flat_p, self.flat_g = torch.zeros(n), torch.zeros(n)
        self.buckets = [("head", 0, n_head), ("block0", n_head, n)]
        self.grad_hook, self.accumulate_grads, self._side = None, False, None
        self.weights_dirty = False


class _ToyModel(torch.nn.Module):
    """logits = tanh(x @ trunk) @ head.  Parameters and gradients are views of the flat buffers; the trunk's bucket is handed
    from inside backward (the engine's hook), the head's gradients arrive through autograd only."""

    def __init__(self, rank, frozen=False, nan_at=None):
        super().__init__()
        eng = self.engine = _ToyEngine()
        eng.flat_p[:D * V].copy_(torch.randn(D * V, generator=torch.Generator().manual_seed(10 + rank)) * 0.3)
        eng.flat_p[1024:1024 + D * D].copy_(torch.randn(D * D, generator=torch.Generator().manual_seed(20 + rank)) * 0.3)
        self.head = torch.nn.Parameter(eng.flat_p[:D * V].view(D, V))
        self.trunk = torch.nn.Parameter(eng.flat_p[1024:1024 + D * D].view(D, D), requires_grad=not frozen)
        self.head.grad = eng.flat_g[:D * V].view(D, V)
        if not frozen:
            self.trunk.grad = eng.flat_g[1024:1024 + D * D].view(D, D)
            self.trunk.register_post_accumulate_grad_hook(lambda p: eng.grad_hook and eng.grad_hook(1))
        self.micro, self.nan_at = 0, nan_at

    def _trunk_frozen(self):
        return not self.trunk.requires_grad

    def forward(self, x):
        self.micro += 1
        out = torch.tanh(x @ self.trunk) @ self.head
        return out * float("nan") if self.micro - 1 == self.nan_at else out


class _ToyOpt:
    def __init__(self, model, lr=0.5):
        self.engine, self.param_groups, self.max_norm = model.engine, [dict(lr=lr, weight_decay=0.0)], 0.0

    def zero_grad(self):
        self.engine.flat_g.zero_()

    def grad_norm(self):
        return self.engine.flat_g.norm().reshape(1)

    def step(self):
        self.engine.flat_p.sub_(self.param_groups[0]["lr"] * self.engine.flat_g)


def _toy_batches(rank, n, B=4):
    g = torch.Generator().manual_seed(300 + rank)
    return [(torch.randn(B, D, generator=g), torch.randint(0, V, (B,), generator=g)) for _ in range(n)]


def _toy_epoch(model, batches, update_freq, log=None):
    from mem_amd import utils
    from mem_amd.engine_for_finetuning import train_one_epoch
    from mem_amd.parallel import attach_reducer
    gate = attach_reducer(model, model.engine, step_exchange=True)
    if log is not None:
        gate.reducer = _Spy(gate.reducer, log, lambda: model.micro)
    stats = train_one_epoch(None, model, torch.nn.CrossEntropyLoss(), batches, _ToyOpt(model), torch.device("cpu"), 0,
                            utils.NativeScalerWithGradNormCount(), max_norm=0, update_freq=update_freq)
    return gate, stats


def _toy_reference(world, n, update_freq, frozen):
    """What the ranks must hold: rank 0's weights, then per update the mean over the ranks of the accumulated gradients."""
    m0 = _ToyModel(0)
    head, trunk = m0.head.detach().clone(), m0.trunk.detach().clone()
    data = [_toy_batches(r, n) for r in range(world)]
    for u in range(n // update_freq):
        gh, gt = torch.zeros_like(head), torch.zeros_like(trunk)
        for r in range(world):
            for x, y in data[r][u * update_freq:(u + 1) * update_freq]:
                h, t = head.clone().requires_grad_(True), trunk.clone().requires_grad_(True)
                (torch.nn.functional.cross_entropy(torch.tanh(x @ t) @ h, y) / update_freq).backward()
                gh += h.grad / world
                gt += t.grad / world
        head -= 0.5 * gh
        if not frozen:
            trunk -= 0.5 * gt
    return head, trunk


def _worker_loop(rank, world, port, q, update_freq, frozen):
    _init(rank, world, port)
    model = _ToyModel(rank, frozen=frozen)
    n, log = 4, []
    gate, stats = _toy_epoch(model, _toy_batches(rank, n), update_freq, log)
    head, trunk = _toy_reference(world, n, update_freq, frozen)
    ok = torch.allclose(model.head.detach(), head, atol=1e-6) and torch.allclose(model.trunk.detach(), trunk, atol=1e-6)
    # collectives were started in the micro-steps that end in an update only; frozen: bucket 0 alone, once per update
    updates = [m for m in range(1, n + 1) if m % update_freq == 0]
    ok = ok and sorted(set(m for m, _ in log)) == updates
    ok = ok and [k for _, k in log] == ([0] if frozen else [1, 0]) * len(updates)
    ok = ok and gate.last_exchanged == ([0] if frozen else [1, 0]) and model.engine.accumulate_grads is False
    ok = ok and gate.reducer.handles == [] and model.engine.weights_dirty
    both = [torch.empty(2048), torch.empty(2048)]
    dist.all_gather(both, model.engine.flat_p)
    ok = ok and torch.equal(both[0], both[1])
    q.put((rank, bool(ok), float(stats["loss"])))
    dist.destroy_process_group()


@pytest.mark.parametrize("update_freq,frozen", [(1, False), (2, False), (1, True), (2, True)])
def test_train_one_epoch_world2(update_freq, frozen):
    """plain / accumulation (exchange on update micro-steps only) / frozen trunk (head bucket only) / both."""
    res = _run_world2(_worker_loop, update_freq, frozen)
    assert [r[:2] for r in res] == [(0, True), (1, True)], res
    assert res[0][2] == res[1][2]                                  # the meters were averaged over the ranks


def _worker_exit(rank, world, port, q):
    _init(rank, world, port)
    model = _ToyModel(rank, nan_at=2 if rank == 1 else None)       # rank 1's loss is NaN in iteration 2 (the third)
    try:
        _toy_epoch(model, _toy_batches(rank, 5), 1)
    finally:
        q.put((rank, model.micro, model._reducer.reducer.handles == []))


def test_non_finite_loss_on_one_rank_ends_every_rank_in_that_iteration():
    res = _run_world2(_worker_exit, expect_exit=1, timeout=60)
    assert res == [(0, 3, True), (1, 3, True)], res                # both left after their third forward, reducer released


# ---------------------------------------------------------------------------------------------- evaluate over unequal shards
def _eval_shards():
    g = torch.Generator().manual_seed(5)
    mk = lambda b: (torch.randn(b, D, generator=g), torch.randint(0, V, (b,), generator=g))   # noqa: E731
    return [[mk(3), mk(2)], [mk(3)]]                               # rank 0: 5 samples in 2 batches, rank 1: 3 in 1


def _worker_eval(rank, world, port, q):
    _init(rank, world, port)
    from mem_amd.engine_for_finetuning import evaluate
    model = torch.nn.Linear(D, V)
    with torch.no_grad():
        model.weight.copy_(torch.randn(V, D, generator=torch.Generator().manual_seed(9)))
        model.bias.zero_()
    st = evaluate(_eval_shards()[rank], model, torch.device("cpu"))
    q.put((rank, st["acc1"], st["acc5"], st["loss"]))
    dist.destroy_process_group()


def test_evaluate_world2_averages_are_count_weighted():
    res = _run_world2(_worker_eval)
    model = torch.nn.Linear(D, V)
    with torch.no_grad():
        model.weight.copy_(torch.randn(V, D, generator=torch.Generator().manual_seed(9)))
        model.bias.zero_()
        batches = [b for shard in _eval_shards() for b in shard]
        correct = sum(int((model(x).argmax(-1) == y).sum()) for x, y in batches)
        n = sum(len(y) for _, y in batches)
        losses = [float(torch.nn.functional.cross_entropy(model(x), y)) for x, y in batches]
    for _, acc1, acc5, loss in res:
        assert abs(acc1 - 100.0 * correct / n) < 1e-4               # per SAMPLE over both shards (5 + 3), not a mean of ranks
        assert abs(acc5 - 100.0) < 1e-4                             # top-min(5, 4 classes)
        assert abs(loss - sum(losses) / len(losses)) < 1e-6         # per batch (the reference's meter), over all 3 batches
    assert res[0][1:] == res[1][1:]
