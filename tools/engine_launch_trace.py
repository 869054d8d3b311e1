"""Launch trace of ViTEngine: one text line per call the engine makes into mem_amd.ops and per stream-ordering call of its
own (_on_side, _side_read_done, _before_overwrite, _side_join, _bucket_ready, the gradient hook), over a fixed list of
scenarios with fixed host-side drop-path masks.  A line holds the name, the current stream (main / side), every scalar
argument and, for every tensor argument, dtype, shape, strides, storage offset and storage bytes -- no addresses, so the
traces of two checkouts can be compared with diff.  Arguments are bound to the callee's signature first: how a call spells
them (positional, keyword, default left out) does not show.  ops.dropout_params / with_row0 build a host-side struct and
launch nothing: they get no line of their own, the struct's fields appear in the launch that takes it.

The MAE engines (second section) launch on one stream and issue plain torch ops besides (copy_ of a bf16 Linear output into its
fp32 buffer, zero_ / add_ on the padded-head gradients): there every in-place or out= ATen call is recorded as well, as
"aten.<op>" with the same tensor description, through a TorchDispatchMode around the step.

The tokenizer (third section, `tok`) is traced through HipTokenizer's public calls only, construction included; every
scenario ends with a line holding the SHA-256 of the bytes of its ids and logits (the kernels use no atomics: the hashes are
reproducible, and equal between two checkouts that compute the same).

    python tools/engine_launch_trace.py OUT.txt [vit|mae|tok]    # needs the GPU; prints the line count per scenario
"""
import ctypes
import inspect
import itertools
import os
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

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
    if isinstance(v, dict):                                       # the **kw of gemm_nt
        return "{" + ", ".join(f"{k}={fmt(e)}" for k, e in v.items()) + "}"
    if isinstance(v, VE.ViTEngine) or callable(v) or type(v).__name__.startswith("MaeEngine"):
        return "."                                                # self of an engine call; the closure given to _on_side
    return repr(v)


def traced(name, f):
    sig = inspect.signature(f)

    def g(*a, **k):
        ba = sig.bind(*a, **k)
        ba.apply_defaults()
        eng = ENG[0]
        side = getattr(eng, "_side", None) is not None and torch.cuda.current_stream() == eng._side
        LINES.append(f"{name} {'side' if side else 'main'} " + " ".join(f"{n}={fmt(v)}" for n, v in ba.arguments.items()))
        return f(*a, **k)
    return g


for n, f in list(vars(ops).items()):
    if inspect.isfunction(f) and f.__module__ == ops.__name__ and not n.startswith("_") and n not in ("dropout_params", "with_row0"):
        setattr(ops, n, traced(n, f))
for n in ENGINE_CALLS:
    setattr(VE.ViTEngine, n, traced(n, getattr(VE.ViTEngine, n)))


class TorchWrites(TorchDispatchMode):
    """Every ATen call that writes into one of its arguments (copy_, zero_, add_, out= forms) as a trace line."""
    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func._schema.is_mutable:
            LINES.append(f"aten.{func._schema.name[6:]} " + " ".join(fmt(a) for a in (*args, *(kwargs or {}).values())))
        return func(*args, **(kwargs or {}))


def run(out, name, eng, step, torch_ops=False, **switches):
    """One scenario: set the switches, run step(), restore them; its lines go behind a header with their count."""
    old = {k: getattr(eng, k) for k in switches}
    for k, v in switches.items():
        setattr(eng, k, v)
    ENG[0], LINES[:] = eng, []
    eng.grad_hook = traced("grad_hook", lambda bucket: None)
    if torch_ops:
        with TorchWrites():
            step()
    else:
        step()
    torch.cuda.synchronize()
    for k, v in old.items():
        setattr(eng, k, v)
    out.write(f"## {name} {switches}: {len(LINES)} lines\n" + "\n".join(LINES) + "\n")
    print(f"{len(LINES):5d}  {name} {switches}")


def vit_section(out):
    from mem_amd.modeling_finetune import ft_vit
    from mem_amd.modeling_pretrain import pt_vit
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s: (torch.rand(*s, generator=g) > 0.3).float()   # noqa: E731
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


def mae_section(out):
    """Two optimizer steps per scenario (forward_loss, backward, grad_norm, FlatAdamW.step): the second one runs sync_weights
    after an update.  Tiny config: 64-wide encoder heads, 32-wide (padded) decoder heads, two blocks per stack."""
    import contextlib
    import io
    from mem_amd.modeling_mae import MaskedAutoencoderViT, mae_vit_base_patch16_dec512d8b
    from mem_amd.optim_factory import FlatAdamW, get_parameter_groups
    from oracle.mae_ref import TINY_MAE, mae_inputs

    def scenario(name, build, precision, imgs, noise, gelu_dg=True, **switches):
        with contextlib.redirect_stdout(io.StringIO()):
            torch.manual_seed(3)
            m = build()
            m.precision = precision
            m = m.cuda().train()
            opt = FlatAdamW(m, get_parameter_groups(m, 0.05, m.no_weight_decay()), lr=1e-4)
        opt.max_norm = 3.0
        eng = m.engine
        if not gelu_dg:
            eng.set_gelu_dg(False)
        imgs, noise = imgs.cuda(), noise.cuda()

        def step():
            for _ in range(2):
                m.forward_loss(imgs, noise=noise)
                m.backward()
                eng.grad_norm()
                opt.step()
        run(out, name, eng, step, torch_ops=True, **switches)
    imgs, noise = mae_inputs(TINY_MAE, 4, 21)
    for mode in (True, False):
        scenario(f"mae tiny fp32 masked_only={mode}", lambda: MaskedAutoencoderViT(**dict(TINY_MAE, LOSS_ONLY_MASKED_MAE=mode)),
                 "fp32", imgs, noise)
    tiny = lambda: MaskedAutoencoderViT(**dict(TINY_MAE, LOSS_ONLY_MASKED_MAE=True))   # noqa: E731
    for fuse in (True, False):
        scenario("mae tiny bf16", tiny, "bf16", imgs, noise, FUSE_LN_BRANCH=fuse)
    scenario("mae tiny bf16 gelu_dg=False", tiny, "bf16", imgs, noise, gelu_dg=False)
    imgs, noise = mae_inputs(dict(img_size=224, patch_size=16), 2, 33)
    scenario("mae base bf16", lambda: mae_vit_base_patch16_dec512d8b(norm_pix_loss=0, LOSS_ONLY_MASKED_MAE=True, img_size=224),
             "bf16", imgs, noise)


def tok_section(out):
    """HipTokenizer on the tiny tokenizer config at B = 6, every precision: fp32, bf16, fp16x2 raw, fp16x2 certified with a kappa
    that flags every sample and a recompute capacity of 4 (two dynamic-batch rounds), and one audited call."""
    import hashlib
    from mem_amd.vae_model import DiscreteVAE, HipTokenizer
    from oracle.vae_ref import TINY_VAE, fill_vae_by_name, vae_inputs
    B = 6
    m = DiscreteVAE(**TINY_VAE).eval()
    m.load_state_dict(fill_vae_by_name(m.state_dict(), seed=0))
    m = m.cuda()
    img = vae_inputs(TINY_VAE, B, 11).cuda()
    sha = lambda t: hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()   # noqa: E731
    for name, kw in (("fp32", {}), ("bf16", dict(precision="bf16")), ("fp16x2 raw", dict(precision="fp16x2", certify=False)),
                     ("fp16x2 certified, every sample flagged", dict(precision="fp16x2", kappa=1e9, exact_capacity=4, audit_every=0)),
                     ("fp16x2 audited", dict(precision="fp16x2", audit_every=1))):
        ENG[0], LINES[:] = None, []
        tok = HipTokenizer(m, max_batch=B, **kw)
        tok.get_codebook_indices(img)
        torch.cuda.synchronize()
        M = B * tok.hw_out[0] * tok.hw_out[1]
        LINES.append(f"sha256 ids={sha(tok.ids[:M])} logits={sha(tok.logits[:M])}")
        out.write(f"## tok {name} {kw}: {len(LINES)} lines\n" + "\n".join(LINES) + "\n")
        print(f"{len(LINES):5d}  tok {name}")


if __name__ == "__main__":
    with open(sys.argv[1], "w") as out:
        for section in (sys.argv[2:] or ["vit", "mae", "tok"]):
            {"vit": vit_section, "mae": mae_section, "tok": tok_section}[section](out)
