"""Launch trace of ViTEngine: one text line per call the engine makes into mem_amd.ops and per stream-ordering call of its
own (_on_side, _side_read_done, _before_overwrite, _side_join, _bucket_ready, the gradient hook), over a fixed list of
scenarios with fixed host-side drop-path masks.  A line holds the name, the current stream (main / side), every scalar
argument and, for every tensor argument, dtype, shape, strides, storage offset and storage bytes -- no addresses, so the
traces of two checkouts can be compared with diff.  Arguments are bound to the callee's signature first: how a call spells
them (positional, keyword, default left out) does not show.  ops.dropout_params / with_row0 build a host-side struct and
launch nothing: they get no line of their own, the struct's fields appear in the launch that takes it.

    python tools/engine_launch_trace.py OUT.txt        # needs the GPU; prints the line count per scenario
"""
import ctypes
import inspect
import itertools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mem_amd import ops, vit_engine as VE                      # noqa: E402

LINES, ENG = [], [None]
ENGINE_CALLS = ("_on_side", "_side_read_done", "_before_overwrite", "_side_join", "_bucket_ready")


def fmt(v):
    if isinstance(v, torch.Tensor):
        return (f"{str(v.dtype)[6:]}{list(v.shape)}s{list(v.stride())}+{v.storage_offset()}/{v.untyped_storage().nbytes()}"
                f"{'' if v.is_cuda else '@host'}")
    if isinstance(v, ctypes.Structure):
        return "{" + " ".join(f"{n}={getattr(v, n)!r}" for n, _ in v._fields_) + "}"
    if isinstance(v, (list, tuple)):
        return "[" + ", ".join(fmt(e) for e in v) + "]"
    if isinstance(v, VE.ViTEngine) or callable(v):               # self of an engine call; the closure given to _on_side
        return "."
    return repr(v)


def traced(name, f):
    sig = inspect.signature(f)

    def g(*a, **k):
        ba = sig.bind(*a, **k)
        ba.apply_defaults()
        eng = ENG[0]
        side = eng is not None and eng._side is not None and torch.cuda.current_stream() == eng._side
        LINES.append(f"{name} {'side' if side else 'main'} " + " ".join(f"{n}={fmt(v)}" for n, v in ba.arguments.items()))
        return f(*a, **k)
    return g


for n, f in list(vars(ops).items()):
    if inspect.isfunction(f) and f.__module__ == ops.__name__ and not n.startswith("_") and n not in ("dropout_params", "with_row0"):
        setattr(ops, n, traced(n, f))
for n in ENGINE_CALLS:
    setattr(VE.ViTEngine, n, traced(n, getattr(VE.ViTEngine, n)))


def run(out, name, eng, step, **switches):
    """One scenario: set the switches, run step(), restore them; its lines go behind a header with their count."""
    old = {k: getattr(eng, k) for k in switches}
    for k, v in switches.items():
        setattr(eng, k, v)
    ENG[0], LINES[:] = eng, []
    eng.grad_hook = traced("grad_hook", lambda bucket: None)
    step()
    torch.cuda.synchronize()
    for k, v in old.items():
        setattr(eng, k, v)
    out.write(f"## {name} {switches}: {len(LINES)} lines\n" + "\n".join(LINES) + "\n")
    print(f"{len(LINES):5d}  {name} {switches}")


def main(path):
    from mem_amd.modeling_finetune import ft_vit
    from mem_amd.modeling_pretrain import pt_vit
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s: (torch.rand(*s, generator=g) > 0.3).float()   # noqa: E731
    out = open(path, "w")
    # ---- pretraining model: 3 blocks at ViT-B width, drop probabilities 0 / 0.15 / 0.3 (block 0 never drops)
    B = 8
    m = pt_vit(img_size=(224, 224), patch_size=(16, 16), in_chans=2, vocab_size=8192, embed_dim=768, depth=3, num_heads=12,
               mlp_ratio=4, drop_path_rate=0.3, use_shared_rel_pos_bias=True, use_abs_pos_emb=False, init_values=0.1).cuda().train()
    eng = m.engine
    x = torch.rand(B, 2, 224, 224, generator=g).cuda()
    pos = torch.zeros(B, eng.L, dtype=torch.bool)
    for b in range(B):
        pos[b, torch.randperm(eng.L, generator=g)[:98 - b % 3]] = True
    labels = torch.randint(0, 8192, (int(pos.sum()),), generator=g).cuda()
    x, mask_u8, rows = m._prep(x, pos.cuda(), False)
    mk_a, mk_b = rnd(6, B), rnd(6, B)
    mk_a[2], mk_a[3], mk_a[4] = 1.0, (torch.arange(B) == 5).float(), 0.0      # keeps everything / drops most / drops every sample
    mk_b[3], mk_b[5] = 0.0, 0.0                                               # the MLP branches that drop every sample
    modes = dict(none=(None, True), masked_a=(mk_a.cuda(), False), masked_b=(mk_b.cuda(), False), skip_a=(mk_a, True),
                 skip_b=(mk_b, True))

    def pt_step(mode):
        dp, skip = modes[mode]
        eng.dp_skip = skip
        eng.forward(x, mask_u8, rows, labels=labels, dp_masks=dp)
        eng.backward()
    for mode, fuse, tail in itertools.product(modes, (True, False), (True, False)):
        run(out, f"pt {mode}", eng, lambda: pt_step(mode), fuse_ln_branch=fuse, tail_rows=tail)
    for mode, level in itertools.product(("none", "masked_a", "skip_a", "skip_b"), (0, 1, 2)):
        run(out, f"pt {mode}", eng, lambda: pt_step(mode), wgrad_group=level)
    for mode in ("masked_a", "skip_a", "skip_b"):
        run(out, f"pt {mode}", eng, lambda: pt_step(mode), accumulate_grads=True)
    del m, eng
    # ---- finetuning model: 3 blocks at ViT-B width, drop probabilities 0 / 0.1 / 0.2, dropout 0.1
    B = 160                                                    # (the two-stream split needs a second part of >= 4096 rows)
    m = ft_vit(img_size=(224, 224), patch_size=(16, 16), in_chans=3, num_classes=11, embed_dim=768, depth=3, num_heads=12,
               mlp_ratio=4, drop_path_rate=0.2, drop_rate=0.1, init_values=0.1, use_abs_pos_emb=False, use_rel_pos_bias=True,
               use_shared_rel_pos_bias=False, use_mean_pooling=True, init_scale=0.001).cuda().train()
    eng = m.engine
    x = torch.rand(B, 3, 224, 224, generator=g).cuda()
    mk = rnd(6, B)
    mk[3] = 0.0
    dxl = torch.randn(B * eng.T, eng.D, generator=g).cuda()
    key = (0x1234567, 0x89ABCDE)

    def ft_step(skip, dk, keep=True):
        eng.dp_skip = skip
        eng.forward_trunk(x, None, mk if skip else mk.cuda(), drop_key=dk, keep=keep)
        if keep:
            eng.backward_trunk(dxl)
    for skip, dk, fuse in itertools.product((False, True), (None, key), (True, False)):
        run(out, f"ft {'skip' if skip else 'masked'} dropout={dk is not None}", eng, lambda: ft_step(skip, dk), fuse_ln_branch=fuse)
    for dk in (None, key):
        run(out, f"ft masked dropout={dk is not None}", eng, lambda: ft_step(False, dk), fwd_two_streams=True)
    for skip in (False, True):
        run(out, f"ft {'skip' if skip else 'masked'} dropout=True keep=False", eng, lambda: ft_step(skip, key, keep=False))
    out.close()


if __name__ == "__main__":
    main(sys.argv[1])
