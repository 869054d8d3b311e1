"""Data-parallel gradient exchange for the flat-buffer engine (replaces the implicit DDP reducer
of /root/reference/mem/run_mem_pretraining.py:365-367 and its C4 parameter broadcast).

One process per GPU, torch.distributed backend "nccl" (= RCCL over xGMI).  The engine lays the
flat gradient buffer out in reverse-layer order, so each bucket (head, block L-1 ... block 0,
embedding) is final the moment backward leaves that layer: ``GradReducer`` is the engine's
``grad_hook`` and enqueues one asynchronous all-reduce per bucket right there.  RCCL runs them on
its own stream behind an event on the CURRENT stream of the call -- the engine calls the hook with its
weight-gradient (side) stream current, after that stream has waited for the main stream's position
(``ViTEngine._bucket_ready``), so the collective is ordered behind every writer of the bucket while
the main stream never waits for a weight gradient -- i.e. overlapped with the rest of backward;
``finish()`` joins them before the gradient norm / AdamW.  ~30 MB fp32 per ViT-B block: large
enough for xGMI link bandwidth, small enough to pipeline 14 messages per step.
Mean semantics (SUM / world) == DDP.  Works on CPU tensors with gloo for the CPU tests.

Options (both off by default = the reference's fp32 DDP exchange):
  * ``bucket_dtype=torch.bfloat16``: a bucket is rounded to bf16, pre-divided by the world size, summed over the ranks in
    bf16 and widened back (torch's bf16_compress_hook arithmetic): 184 MB instead of 367 MB per ViT-B step on the wire;
  * ``reserve_cus=k``: while buckets are in flight the library sizes the persistent one-workgroup-per-CU grids (GEMMs,
    attention) it launches ON THIS ENGINE'S STREAMS for k CUs fewer (``memhip_stream_reserve_cus``: scoped to the stream
    handles, another engine of the process is not affected), so that RCCL's channel kernels find CUs of their own instead
    of displacing workgroups of a grid that covers the whole chip (whose stragglers then run a second round).  The
    reservation is dropped by ``finish()`` / ``release()``; the training loops call ``release()`` on every exit path.
    No measurement on more than one GPU exists yet: the entrypoint leaves it at 0.

``attach_reducer`` is what both entrypoints call (broadcast, hook, stale bf16 shadows).  The finetuning loop has modes the
pretraining loop has not -- gradient accumulation, a frozen trunk whose backward the engine never enters -- and gets the
reducer behind a ``StepExchange``: the same object to the engine (``grad_hook``) and to the scaler (``finish`` /
``sync_flag``), which decides per micro-step whether a bucket is exchanged and hands over what the engine did not.
"""
import os

import torch
import torch.distributed as dist


class GradReducer:
    def __init__(self, flat_g, buckets, flat_p=None, group=None, coalesce_small=0, force=False, bucket_dtype=None,
                 reserve_cus=0, streams=None):
        """streams: callable returning the torch.cuda.Stream objects the engine launches on (main + side stream): the CU
        reservation is set on exactly these."""
        self.flat_g, self.buckets, self.group = flat_g, buckets, group
        self._streams_fn, self._res_streams = streams, []
        self.bucket_dtype = bucket_dtype if bucket_dtype not in (None, torch.float32) else None
        self.reserve_cus = int(reserve_cus)
        self._reserved = False
        self.wire = torch.empty_like(flat_g, dtype=self.bucket_dtype) if self.bucket_dtype is not None else None
        esz = 2 if self.bucket_dtype is not None else 4
        self.bytes_per_step = sum(b1 - b0 for _, b0, b1 in buckets) * esz
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        # force: issue the collectives even in a one-rank group (single-GPU dry run of the RCCL path: bench.py
        # with MEMHIP_BENCH_FORCE_DIST=1)
        self.active = (self.world > 1 or force) and dist.is_initialized()
        self.handles = []
        # RCCL (ncclAvg, RCCL >= 2.10) averages inside the collective; gloo (CPU tests) has no AVG: SUM, then divide
        # on the compute stream after the join (one extra pass over the buckets)
        self.use_avg = dist.is_initialized() and dist.get_backend(group) == "nccl"
        if flat_p is not None and self.active:
            dist.broadcast(flat_p, src=0, group=group)          # rank-0 weights everywhere (DDP ctor)

    def _reserve(self, on):
        if self.reserve_cus > 0 and self._reserved != on and self.flat_g.is_cuda:
            from . import ops
            if on:
                self._res_streams = [s for s in (self._streams_fn() if self._streams_fn else [torch.cuda.current_stream()])
                                     if s is not None]
            for s in self._res_streams:
                ops.stream_reserve_cus(s, self.reserve_cus if on else 0)
            self._reserved = on

    def release(self):
        """Drop the CU reservation and forget pending handles (exception / early-return paths of a training loop)."""
        self._reserve(False)
        self.handles = []

    def __del__(self):
        try:
            self._reserve(False)
        except Exception:
            pass

    def __call__(self, bucket_index):
        if not self.active:
            return
        self._reserve(True)                       # from the first bucket of a step until finish()
        _, b0, b1 = self.buckets[bucket_index]
        view = self.flat_g[b0:b1]
        if self.wire is not None:
            w = self.wire[b0:b1]
            # pre-divide in fp32, ONE rounding to bf16 (the division writes straight into the preallocated wire buffer: no
            # fp32 temporary of the bucket's size per call), then a bf16 SUM over the ranks
            torch.div(view, self.world, out=w)
            h = dist.all_reduce(w, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
            self.handles.append((h, (view, w)))
            return
        if self.use_avg:
            h = dist.all_reduce(view, op=dist.ReduceOp.AVG, group=self.group, async_op=True)
            self.handles.append((h, None))
        else:
            h = dist.all_reduce(view, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
            self.handles.append((h, view))

    def sync_flag(self, flag):
        """MAX of a small integer / float flag tensor over the ranks, in place (the bad-sample counter of the training loop:
        every rank must take the SAME skip-this-update decision and every rank must raise at the next check -- a rank-local
        flag would let the replicas diverge).  No-op outside a multi-rank group."""
        if self.active and self.world > 1:
            dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=self.group)
        return flag

    def finish(self):
        for h, view in self.handles:
            h.wait()
            if isinstance(view, tuple):            # bf16 wire buffer -> the fp32 gradient
                view[0].copy_(view[1])
            elif view is not None:
                view.div_(self.world)
        self.handles = []
        self._reserve(False)


class StepExchange:
    """The reducer as the finetuning loop drives it (engine_for_finetuning.train_one_epoch); reducer-shaped, so it is the
    engine's ``grad_hook`` and the scaler's ``reducer=`` at once.

    * Accumulation (``update_freq`` > 1): micro-batch gradients ADD into ``flat_g``; a bucket averaged on a non-final
      micro-step and then added to would be wrong.  ``begin_micro_step(do_update)`` arms the hook for the micro-step that
      ends in an update only; the buckets are exchanged there, on the accumulated buffer (DDP ``no_sync`` arithmetic: the mean
      is linear, so it equals reducing every micro-step).
    * Buckets the engine never hands over: with a frozen trunk ``backward_trunk`` is not entered and the head / fc_norm
      gradients come from torch autograd through the parameter views.  ``finish()`` -- called by the scaler after
      ``loss.backward()`` on update steps only -- first hands every EXPECTED bucket that was not handed in this step to the
      reducer, in index order (the same set in the same order on every rank), then joins.  ``expected`` is every bucket,
      or bucket 0 (the head) alone for a frozen trunk: nothing of the trunk's range of ``flat_g`` is read or written."""

    def __init__(self, reducer, frozen=False):
        self.reducer = reducer
        self.armed = True
        self.handed = []                          # bucket indices given to the reducer in this step, in order
        self.last_exchanged = []                  # ... in the last finished step
        self.set_frozen(frozen)

    def set_frozen(self, frozen):
        self.frozen = bool(frozen)
        self.expected = [0] if self.frozen else list(range(len(self.reducer.buckets)))

    @property
    def bytes_per_step(self):
        """Wire bytes of one update step: the expected buckets, in the reducer's element size."""
        esz = 2 if self.reducer.bucket_dtype is not None else 4
        return sum(self.reducer.buckets[k][2] - self.reducer.buckets[k][1] for k in self.expected) * esz

    def begin_micro_step(self, do_update):
        self.armed = bool(do_update)
        self.handed = []

    def __call__(self, bucket_index):
        if not self.armed:
            return                                # an accumulating micro-step: no collective is started
        if bucket_index in self.handed:
            raise RuntimeError(f"bucket {bucket_index} handed to the gradient exchange twice in one step")
        self.handed.append(bucket_index)
        self.reducer(bucket_index)

    def hand_missing(self):
        """Every expected bucket the engine has not handed in this step, once, in index order; returns them."""
        missing = [k for k in self.expected if k not in self.handed]
        for k in missing:
            self(k)
        return missing

    def finish(self):
        self.hand_missing()
        self.reducer.finish()
        self.last_exchanged, self.handed = self.handed, []

    def sync_flag(self, flag):
        return self.reducer.sync_flag(flag)

    def release(self):
        self.reducer.release()
        self.handed, self.armed = [], True


def any_rank(reducer, flag, device="cpu"):
    """True on EVERY rank when ``flag`` is true on any (MAX over the ranks through ``reducer.sync_flag``): a loop that leaves
    on a rank-local condition -- a non-finite loss -- would strand the other ranks in the next collective."""
    if reducer is None:
        return bool(flag)
    t = torch.tensor([1 if flag else 0], dtype=torch.int32, device=device)
    return bool(int(reducer.sync_flag(t).item()))


def attach_reducer(model, eng, step_exchange=False):
    """What an entrypoint does once the process group exists and before anything copies the weights (optimizer, EMA twin): the
    reducer over the engine's flat buffers (its constructor broadcasts rank 0's ``flat_p``), as ``model._reducer`` and the
    engine's ``grad_hook``; the bf16 shadows are stale after the broadcast.  ``step_exchange``: behind a StepExchange (the
    finetuning loop).  reserve_cus > 0 leaves CUs to RCCL's channel kernels while buckets are in flight; no measurement on
    more than one GPU exists yet, so the default is 0 -- MEMHIP_RESERVE_CUS=16 tries it."""
    red = GradReducer(eng.flat_g, eng.buckets, flat_p=eng.flat_p,
                      reserve_cus=int(os.environ.get("MEMHIP_RESERVE_CUS", "0")),
                      streams=lambda: [torch.cuda.current_stream(), eng._side])
    if step_exchange:
        frozen = getattr(model, "_trunk_frozen", None)
        red = StepExchange(red, frozen=bool(frozen()) if frozen is not None else False)
    model._reducer = red
    eng.grad_hook = red
    eng.weights_dirty = True
    return red
