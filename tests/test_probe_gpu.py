"""-m gpu: frozen-backbone probing and the forward-only engine mode on the device -- memhip_pool_tokens / _bwd against
float64, forward_trunk(keep=False) bit-equal to keep=True, evaluation parity with the torch mean it replaces, five frozen
training steps against a torch head-only reference, the forward-only memory footprint, and the stage-3 entrypoint."""
import contextlib
import copy
import gc
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24            # unit roundoff of fp32 (round to nearest)


# ------------------------------------------------------------------ the pooling kernels
def _pool_bound(x64, ref):
    """|out - ref| <= (T-1) * 2^-24 * mean_t|x| + 2^-24 * |ref| per element: the first term is the worst case of a
    SEQUENTIAL fp32 sum of the T-1 rows ((n-1) u sum|x|, over n) -- any summation tree is tighter --, the second the one
    rounding of the division."""
    T = x64.shape[1]
    return (T - 1) * U * x64[:, 1:].abs().mean(1) + U * ref.abs()


@pytest.mark.parametrize("B,T,D,offset", [(1, 2, 64, 0.0), (3, 197, 768, 0.0), (2, 321, 1024, 0.0), (5, 1201, 1024, 0.0),
                                          (256, 197, 768, 0.0), (3, 197, 768, 1e3)])
def test_pool_tokens_against_float64(B, T, D, offset):
    from mem_amd import ops
    g = torch.Generator().manual_seed(B * 7919 + T)
    x = (torch.randn(B * T, D, generator=g) + offset).cuda()
    out = ops.pool_tokens(x, B, T)
    out2 = ops.pool_tokens(x, B, T)
    torch.cuda.synchronize()
    x64 = x.double().view(B, T, D)
    ref = x64[:, 1:].mean(1)
    err = (out.double() - ref).abs()
    bound = _pool_bound(x64, ref)
    print("pool_tokens (%d, %d, %d) offset %g: max err %.3e, min bound %.3e, max err / bound %.4f"
          % (B, T, D, offset, err.max().item(), bound.min().item(), (err / bound).max().item()))
    assert bool((err <= bound).all())
    assert torch.equal(out, out2)                                               # fixed summation order: run-to-run bit-equal


@pytest.mark.parametrize("B,T,D,ldx", [(3, 50, 96, 128), (2, 7, 70, 70), (4, 197, 66, 67)])
def test_pool_tokens_strided_and_unaligned_rows(B, T, D, ldx):
    """ldx > D (a column block of a wider matrix) and widths / strides that rule out 16-byte lane loads: same bound; the
    columns behind D are never read into the result and nothing behind out[B, D] is written."""
    from mem_amd import ops
    g = torch.Generator().manual_seed(T * 31 + D)
    big = torch.randn(B * T, ldx, generator=g).cuda()
    big[:, D:] = float("nan")
    x = big[:, :D]
    guard = torch.full((B + 1, D), 7.0, device="cuda")
    out = ops.pool_tokens(x, B, T, out=guard[:B])
    torch.cuda.synchronize()
    x64 = x.double().reshape(B, T, D)
    ref = x64[:, 1:].mean(1)
    assert bool(((out.double() - ref).abs() <= _pool_bound(x64, ref)).all())
    assert bool((guard[B] == 7.0).all())


@pytest.mark.parametrize("B,T,D", [(1, 2, 64), (3, 197, 768), (2, 321, 1024), (5, 1201, 1024), (256, 197, 768), (3, 9, 70)])
def test_pool_tokens_bwd_equals_the_division(B, T, D):
    """dx = dout[:, None, :] / (T - 1) on the token rows and 0 on the cls row, bit for bit, every element written (dx starts
    as NaN).  The kernel divides (IEEE); the expected value is formed on the host, where torch's division by a scalar is a
    division as well (on the device torch multiplies by the rounded reciprocal of a scalar divisor)."""
    from mem_amd import ops
    g = torch.Generator().manual_seed(B + T + D)
    dout = torch.randn(B, D, generator=g)
    dx = torch.full((B * T, D), float("nan"), device="cuda")
    ops.pool_tokens_bwd(dout.cuda(), T, dx=dx)
    torch.cuda.synchronize()
    want = (dout[:, None, :] / (T - 1)).expand(B, T, D).clone()
    want[:, 0] = 0.0
    assert torch.equal(dx.view(B, T, D).cpu(), want)


# ------------------------------------------------------------------ forward-only engine mode
def _cfg(size, rel):
    from oracle.gen_golden_ft import FT_A
    cfg = dict(FT_A, drop_path_rate=0.2, drop_rate=0.1)
    if size == "vitb4":
        cfg.update(img_size=(224, 224), embed_dim=768, depth=4, num_heads=12)
    if rel == "shared":
        cfg.update(use_rel_pos_bias=False, use_shared_rel_pos_bias=True, use_abs_pos_emb=True)
    return cfg


def _model(cfg, seed=3):
    from mem_amd.modeling_finetune import ft_vit
    from oracle.vit_ref import fill_by_name
    m = ft_vit(**cfg)
    m.load_state_dict(fill_by_name(m.state_dict(), seed=seed))
    return m.cuda()


@pytest.mark.parametrize("rel", ["block", "shared"])
@pytest.mark.parametrize("size,B", [("tiny", 6), ("vitb4", 48)])
def test_forward_only_stream_is_bit_equal_to_the_training_forward(size, B, rel):
    """forward_trunk(keep=False) against keep=True on the same engine: plain, drop-path masks in the work-skipping and
    in the masked form, element-wise dropout with a fixed key, both together; per-block and shared bias tables (the
    shared form also carries the abs. position embedding).  Both orders (the rotation runs on clean and on used buffers)."""
    from oracle.gen_golden_ft import ft_inputs
    cfg = _cfg(size, rel)
    m = _model(cfg).train()
    eng = m.engine
    depth = cfg["depth"]
    x = ft_inputs(cfg, B, 7)[0].cuda()
    masks = (torch.rand(2 * depth, B, generator=torch.Generator().manual_seed(2)) > 0.3).float()
    masks[3] = 0.0                                             # block 1's MLP branch: every sample drops it
    key = (0x1234567, 0x89ABCDE)
    first = eng.forward_trunk(x, None, None, keep=False).clone()                    # before any training forward
    assert len(eng.x) == 3 and len(eng.act) == 1 and eng.B_stash == 0 and not hasattr(eng, "dx")
    for name, dp, skip, dk in (("plain", None, True, None), ("dp_skip", masks, True, None), ("dp_masked", masks.cuda(), False, None),
                               ("dropout", None, True, key), ("dropout_dp_skip", masks, True, key),
                               ("dropout_dp_masked", masks.cuda(), False, key)):
        eng.dp_skip = skip
        a = eng.forward_trunk(x, None, dp, drop_key=dk, keep=False).clone()
        assert not eng.cur["keep"] and (eng.cur["plan"] is not None) == (dp is not None and skip), name
        b = eng.forward_trunk(x, None, dp, drop_key=dk, keep=True).clone()
        c = eng.forward_trunk(x, None, dp, drop_key=dk, keep=False).clone()
        torch.cuda.synchronize()
        assert torch.isfinite(b).all(), name
        assert torch.equal(a, b), name
        assert torch.equal(c, b), name
        if name == "plain":
            assert torch.equal(first, b)
    assert len(eng.x) == 2 * depth + 1 and len(eng.act) == depth and eng.B_stash == eng.B


def test_forward_only_two_stream_split_is_bit_equal():
    from oracle.gen_golden_ft import ft_inputs
    cfg = dict(_cfg("vitb4", "block"), depth=2, drop_path_rate=0.0)
    B = 160                                                    # (the two-stream split needs a second part of >= 4096 rows)
    m = _model(cfg).train()
    eng = m.engine
    x = ft_inputs(cfg, B, 7)[0].cuda()
    key = (5, 6)
    one = eng.forward_trunk(x, None, None, drop_key=key, keep=False).clone()
    eng.fwd_two_streams = True
    assert 0 < eng._split_point(B) < B
    two = eng.forward_trunk(x, None, None, drop_key=key, keep=False).clone()
    torch.cuda.synchronize()
    assert torch.equal(one, two)
    assert eng.B_stash == 0


def test_backward_after_a_forward_only_pass_raises():
    from oracle.gen_golden_ft import FT_A, ft_inputs
    m = _model(FT_A).train()
    eng = m.engine
    x = ft_inputs(FT_A, 4, 1)[0].cuda()
    xl = eng.forward_trunk(x, None, None, keep=False)
    with pytest.raises(RuntimeError, match="keep=False"):
        eng.backward_trunk(torch.zeros_like(xl))
    eng.forward_trunk(x, None, None, keep=True)
    eng.backward_trunk(torch.zeros_like(xl))                                    # and the training path still runs
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match="forward-only"):
        eng.forward_trunk(x, None, None, tail_rows=torch.zeros(1, dtype=torch.int32, device="cuda"), keep=False)


# ------------------------------------------------------------------ evaluation parity
@pytest.mark.parametrize("size,B", [("tiny", 6), ("vitb4", 16)])
def test_eval_logits_against_the_torch_mean_they_replace(size, B):
    """model.eval() logits (pool_tokens on the engine's buffer) against fc_norm(x[:, 1:].mean(1)) -> head on the keep=True
    stream under the same autocast.  The streams are bit-equal, so the only difference is the fp32 summation order of the
    mean: both pooled vectors lie within e (the bound of test_pool_tokens_against_float64) of the exact mean, |dp| <= 2 e.
    Pushed through the tail, to first order in dp:
      fc_norm (fp32 LayerNorm): its Jacobian is diag(w) (I - 11'/D - y y'/D) / sigma, spectral norm <= max|w| / sigma, so
        |dy_d| <= ||dy||_2 <= max|w| ||dp||_2 / sigma; plus, for the roundings inside the two evaluations (the mean and the
        centred value carry a few u of |p_d| + |mu|, the scale and the affine a few u of the result),
        8 u (|w_d| (|p_d| + |mu|) / sigma + |y_d| + |b_d|)
      head (bf16 GEMM, fp32 accumulate, same kernel and order): y is rounded to bf16 first, a changed y may round the other
        way: |d bf16(y_d)| <= |dy_d| + 2^-7 |y_d|; |dlogit_c| <= sum_d |W16_cd| |d bf16(y_d)|, and the bf16 rounding of the
        result may flip as well: + 2^-7 |logit_c|.
    The 2^-7 terms dominate, so this bound is NOT sharp: it shows that the pooled path computes the same head, not that no
    token row was dropped -- that is test_pool_tokens_against_float64's job, whose bound is tight."""
    from oracle.gen_golden_ft import ft_inputs
    cfg = dict(_cfg(size, "block"), drop_rate=0.0)
    m = _model(cfg).eval()
    eng = m.engine
    x = ft_inputs(cfg, B, 5)[0].cuda()
    T, D = eng.T, eng.D
    with torch.no_grad():
        lo_new = m(x).float()
        assert eng.B_stash == 0
        xl = eng.forward_trunk(x, None, None, keep=True)[: B * T].view(B, T, D).clone()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            p_old = xl[:, 1:, :].mean(1)
            y_old = m.fc_norm(p_old)
            lo_old = m.head(y_old).float()
    x64 = xl.double()
    e = _pool_bound(x64, x64[:, 1:].mean(1))                                    # [B, D]
    dp = 2.0 * e
    w, b = m.fc_norm.weight.double(), m.fc_norm.bias.double()
    sigma = (p_old.double().var(1, unbiased=False) + m.fc_norm.eps).sqrt()       # [B]
    p64 = p_old.double()
    dy = (w.abs().max() * dp.norm(dim=1) / sigma)[:, None] + 8 * U * (
        w.abs()[None, :] * (p64.abs() + p64.mean(1, keepdim=True).abs()) / sigma[:, None] + y_old.double().abs() + b.abs()[None, :])
    dy16 = dy + 2.0 ** -7 * y_old.double().abs()
    w16 = m.head.weight.detach().to(torch.bfloat16).double().abs()               # [V, D]
    bound = dy16 @ w16.t() + 2.0 ** -7 * lo_old.double().abs()
    diff = (lo_new.double() - lo_old.double()).abs()
    print("eval parity %s B=%d: max |dlogit| %.3e (max |logit| %.3e), min bound %.3e, max diff / bound %.4f"
          % (size, B, diff.max().item(), lo_old.abs().max().item(), bound.min().item(), (diff / bound).max().item()))
    assert bool((diff <= bound).all())
    # forward_features under eval(): the pooled, normed features [B, D]
    with torch.no_grad():
        f = m.forward_features(x)
    assert f.shape == (B, D) and bool(((f.double() - y_old.double()).abs() <= dy).all())


# ------------------------------------------------------------------ frozen training
class _CE(torch.nn.Module):
    def forward(self, out, target):
        return torch.nn.functional.cross_entropy(out.float(), target)


def _probe_optimizer(m, lr):
    from mem_amd import optim_factory as OF
    depth = m.get_num_layers()
    assigner = OF.LayerDecayValueAssigner(list(0.75 ** (depth + 1 - i) for i in range(depth + 2)))

    class OA:
        opt = "adamw"; weight_decay = 0.05; opt_eps = 1e-8
    OA.lr = lr
    with contextlib.redirect_stdout(io.StringIO()):
        return OF.create_optimizer(OA(), m, skip_list=m.no_weight_decay(), get_num_layer=assigner.get_layer_id,
                                   get_layer_scale=assigner.get_scale)


@pytest.mark.parametrize("update_freq", [1, 2])
def test_frozen_training_against_a_torch_head_reference(update_freq):
    """Five optimizer steps of train_one_epoch on a frozen tiny ft_vit (layer decay, drop path 0.1, clipping): the trunk's
    masters, bf16 shadows and transposed copies stay bit-equal, its gradient range stays zero, no stash is allocated; the
    losses and head / fc_norm weights follow a torch reference that takes the engine's pooled features (captured at
    fc_norm's input) as constants: fc_norm -> head -> criterion -> clip -> torch.optim.AdamW with the same groups.
    Weights: rtol 2e-5 / atol 2e-6 (the bar of test_finetune_layer_decay_adamw_vs_torch).  Loss: the fp32 CE of bf16 logits is
    2-Lipschitz in max|dlogit|; the two heads differ by <= 2e-5 relative, which can flip the bf16 rounding of a weight
    (2^-8), of a normed feature (2^-8) and of the logit (2^-7): |dloss| <= 2 * 2^-6 * max_c(sum_d |W_cd| |y_d| + |b_c|).
    That loss bound is a worst case and far above the differences seen (the ratio is printed); the weight comparison after
    five steps is the sharp part of this test."""
    from mem_amd import engine_for_finetuning as EF
    from mem_amd.utils import NativeScalerWithGradNormCount
    from oracle.gen_golden_ft import FT_A, ft_inputs
    cfg = dict(FT_A, num_classes=4, drop_path_rate=0.1)
    torch.manual_seed(0)
    m = _model(cfg, seed=6)
    frozen = m.freeze_backbone()
    lr, clip, steps = 2e-3, 1.0, 5
    opt = _probe_optimizer(m, lr)
    eng = m.engine
    he = eng.head_end
    assert opt._active_end == he < eng.nflat
    tail_names = [n for n, p in m.named_parameters() if p.requires_grad]
    assert sorted(tail_names) == ["fc_norm.bias", "fc_norm.weight", "head.bias", "head.weight"]
    # the reference tail: copies of fc_norm / head with the optimizer's groups
    r_norm, r_head = copy.deepcopy(m.fc_norm), copy.deepcopy(m.head)
    r_named = {"fc_norm.weight": r_norm.weight, "fc_norm.bias": r_norm.bias, "head.weight": r_head.weight, "head.bias": r_head.bias}
    for k, p in r_named.items():
        p.data = p.data.clone()
        p.grad = None
    name_of = {id(p): n for n, p in m.named_parameters()}
    lr_sched = [lr * (0.5 + 0.1 * i) for i in range(steps)]
    tgroups = [{"params": [r_named[name_of[id(p)]] for p in g["params"]], "weight_decay": g["weight_decay"]} for g in opt.param_groups]
    assert all(g["lr_scale"] == 1.0 for g in opt.param_groups)
    topt = torch.optim.AdamW(tgroups, lr=lr, betas=(0.9, 0.95), eps=1e-8)
    eng.sync_weights()
    p0, w0 = eng.flat_p.clone(), eng.flat_w16.clone()
    wt0 = {(i, k): v.clone() for i, d in eng.wT.items() for k, v in d.items()}
    start = {n: p.detach().clone() for n, p in m.named_parameters()}
    data = [ft_inputs(cfg, 8, 100 + i) for i in range(steps * update_freq)]
    feats, seen = [], []
    hook = m.fc_norm.register_forward_hook(lambda mod, inp, out: feats.append(inp[0].detach().clone()))
    step = opt.step

    def checked_step(*a, **k):                                  # what the optimizer consumes (zero_grad() clears it afterwards)
        seen.append((bool((eng.flat_g[he:] == 0).all()), float(eng.flat_g[:he].abs().max())))
        return step(*a, **k)
    opt.step = checked_step
    losses = []
    crit = _CE()
    orig = EF.train_class_batch

    def recording(model, samples, target, criterion):
        loss, out = orig(model, samples, target, criterion)
        losses.append(loss.item())
        return loss, out
    EF.train_class_batch = recording
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            EF.train_one_epoch(None, m, crit, data, opt, torch.device("cuda"), 0, NativeScalerWithGradNormCount(), clip,
                               lr_schedule_values=lr_sched, num_training_steps_per_epoch=steps, update_freq=update_freq)
    finally:
        EF.train_class_batch = orig
        hook.remove()
    torch.cuda.synchronize()
    assert m.training and opt.steps == steps and len(feats) == len(data) == len(losses)
    assert all(f.shape == (8, eng.D) and f.dtype == torch.float32 and not f.requires_grad for f in feats)
    # -- nothing of the trunk moved, nothing of it was produced, nothing for a backward was allocated
    assert torch.equal(eng.flat_p[he:], p0[he:])
    assert torch.equal(eng.flat_w16[he:], w0[he:])
    assert all(torch.equal(eng.wT[i][k], v) for (i, k), v in wt0.items())
    assert all(torch.equal(p.detach(), start[n]) for n, p in m.named_parameters() if n in frozen)
    assert all(not torch.equal(p.detach(), start[n]) for n, p in m.named_parameters() if n in tail_names)
    assert len(seen) == steps and all(z for z, _ in seen) and all(g > 0 for _, g in seen), seen
    assert eng.B_stash == 0 and len(eng.x) == 3 and len(eng.act) == 1
    assert torch.equal(eng.flat_w16[:he].float(), eng.flat_p[:he].to(torch.bfloat16).float())   # the head's shadows follow
    # -- the torch reference on the captured features
    worst = 0.0
    for it in range(steps):
        for g in topt.param_groups:
            g["lr"] = lr_sched[it]
        for k in range(update_freq):
            i = it * update_freq + k
            y = data[i][1].cuda()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                f = r_norm(feats[i])
                lo = r_head(f)
            loss = crit(lo, y)
            s = (f.detach().double().abs() @ r_head.weight.detach().double().abs().t() + r_head.bias.detach().double().abs()).max().item()
            tol = 2.0 * 2.0 ** -6 * s
            worst = max(worst, abs(loss.item() - losses[i]) / tol)
            assert abs(loss.item() - losses[i]) <= tol, (it, k, loss.item(), losses[i], tol)
            (loss / update_freq).backward()
        torch.nn.utils.clip_grad_norm_(list(r_named.values()), clip)
        topt.step()
        topt.zero_grad()
    print("frozen training, update_freq %d: losses %s, worst |dloss| / tol %.3e" % (update_freq, ["%.5f" % v for v in losses], worst))
    for n, p in m.named_parameters():
        if n in tail_names:
            torch.testing.assert_close(p.detach(), r_named[n].detach(), rtol=2e-5, atol=2e-6, msg=lambda s_, n=n: f"{n}: {s_}")


# ------------------------------------------------------------------ memory
def test_forward_only_footprint_and_training_afterwards():
    """A fresh ViT-B ft_vit that only evaluates at B = 128 peaks below 1.15 x (three residual buffers + two activation sets +
    patches + input + parameters), all from the dims; the per-block stash (12 activation sets, 25 snapshots: several times
    that) is never allocated.  A training step afterwards allocates it and gives the loss of a model that never ran
    forward-only, bit for bit."""
    from mem_amd.modeling_finetune import ft_vit
    from oracle.gen_golden_ft import ft_inputs
    cfg = dict(img_size=(224, 224), patch_size=(16, 16), in_chans=3, num_classes=10, embed_dim=768, depth=12, num_heads=12,
               mlp_ratio=4, drop_path_rate=0.0, init_values=0.1, use_abs_pos_emb=False, use_rel_pos_bias=True,
               use_mean_pooling=True)
    B, Bt = 128, 32
    gc.collect()
    torch.cuda.empty_cache()
    torch.manual_seed(0)
    m = ft_vit(**cfg)
    sd = copy.deepcopy(m.state_dict())
    xe, _ = ft_inputs(cfg, B, 1)
    xt, yt = ft_inputs(cfg, Bt, 2)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    m = m.cuda().eval()
    eng = m.engine
    with torch.no_grad():
        for _ in range(2):
            lo = m(xe.cuda())
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    D, Hd, T, L, depth, heads = 768, 3072, 197, 196, 12, 12
    M = B * T
    resid = 3 * (M + T) * D * 4
    act_set = (M + 256) * (6 * D + 2 * Hd) * 2 + B * heads * eng.TP * 4 + 4 * M * 4
    patches = B * L * (3 * 16 * 16) * 2
    inputs = B * 3 * 224 * 224 * 4 + B * L
    nparam = sum(p.numel() for p in m.parameters())
    params = eng.nflat * (4 + 4 + 2) + depth * (4 * D * D + 2 * D * Hd) * 2      # masters, gradients, shadows, transposed copies
    assert eng.nflat <= 1.02 * nparam + 1024 * 400                                 # (padding of the flat layout)
    arith = resid + 2 * act_set + patches + inputs + params
    stash = 12 * act_set + 25 * (M + T) * D * 4
    print("forward-only peak %.1f MB; forward set %.1f MB (x 1.15 = %.1f); the 12-block stash alone would be %.1f MB"
          % (peak / 2 ** 20, arith / 2 ** 20, 1.15 * arith / 2 ** 20, stash / 2 ** 20))
    assert torch.isfinite(lo).all()
    assert peak <= 1.15 * arith, (peak, arith)
    assert eng.B_stash == 0 and len(eng.act) == 1
    # -- a training step afterwards, against a model that never ran forward-only
    crit = torch.nn.CrossEntropyLoss()
    m.train()
    loss_a = crit(m(xt.cuda()).float(), yt.cuda())
    loss_a.backward()
    assert eng.B_stash == B and len(eng.act) == depth
    ga = eng.flat_g.clone()
    m2 = ft_vit(**cfg)
    m2.load_state_dict(sd)
    m2 = m2.cuda().train()
    loss_b = crit(m2(xt.cuda()).float(), yt.cuda())
    loss_b.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss_a) and torch.equal(loss_a, loss_b)
    assert torch.isfinite(ga).all() and float(ga[eng.head_end:].abs().max()) > 0
    cos = torch.dot(ga, m2.engine.flat_g) / (ga.norm() * m2.engine.flat_g.norm())
    assert cos.item() >= 0.9999, cos.item()                                      # (the weight gradients add with atomics)


# ------------------------------------------------------------------ entrypoint
def test_cli_frozen_backbone_then_eval(tmp_path):
    """python -m mem_amd.run_class_finetuning --freeze_backbone 1 in a fresh child process: two epochs, froze / kept lines,
    the trunk of the checkpoint equals the initial one, checkpoint keys equal those of an unfrozen run, --eval reproduces the
    logged accuracy, and a resumed run comes back frozen."""
    from conftest import ROOT
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def base(out):
        return [sys.executable, "-m", "mem_amd.run_class_finetuning", "--expweek", "t", "--data_path", "synthetic", "--nb_classes", "4",
                "--input_H", "64", "--input_W", "96", "--batch_size", "8", "--synthetic_samples", "32", "--num_workers", "0",
                "--transformer_depth", "2", "--transformer_emb", "128", "--transformer_heads", "2", "--rand_aug", "0",
                "--slice_max_evs", "5000", "--output_dir", str(out), "--layer_decay", "0.75", "--lr", "1e-3",
                "--warmup_epochs", "0", "--save_ckpt_freq", "1", "--model_ema_decay", "0.9"]
    out, plain = tmp_path / "probe", tmp_path / "plain"
    out.mkdir(); plain.mkdir()
    r = subprocess.run(base(out) + ["--epochs", "2", "--freeze_backbone", "1"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "froze patch_embed.proj.weight" in r.stdout and "froze blocks.1.mlp.fc2.weight" in r.stdout
    assert "kept head.weight" in r.stdout and "kept fc_norm.bias" in r.stdout and "froze head" not in r.stdout
    assert "Accuracy of the network on the" in r.stdout
    log = [json.loads(l) for l in open(out / "log.txt")]
    assert len(log) == 2 and all(np.isfinite(e["train_loss"]) and "test_acc1" in e for e in log)
    ck0 = torch.load(out / "checkpoint-0.pth", map_location="cpu", weights_only=False)
    ck1 = torch.load(out / "checkpoint-1.pth", map_location="cpu", weights_only=False)
    for k, v in ck1["model"].items():
        tail = k.startswith(("head.", "fc_norm."))
        assert torch.equal(v, ck0["model"][k]) != tail, k                        # the trunk stood still, the head moved
    assert log[0]["n_parameters"] == sum(v.numel() for k, v in ck1["model"].items() if k.startswith(("head.", "fc_norm.")))
    r0 = subprocess.run(base(plain) + ["--epochs", "1"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r0.returncode == 0, r0.stdout[-3000:] + r0.stderr[-3000:]
    assert "froze " not in r0.stdout
    ckp = torch.load(plain / "checkpoint-0.pth", map_location="cpu", weights_only=False)
    assert set(ck1) == set(ckp) and list(ck1["model"]) == list(ckp["model"]) and list(ck1["model_ema"]) == list(ckp["model_ema"])
    r2 = subprocess.run(base(out) + ["--eval", "--freeze_backbone", "1", "--resume", str(out / "checkpoint-1.pth")], cwd=ROOT,
                        env=env, capture_output=True, text=True, timeout=900)
    assert r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-3000:]
    assert "Accuracy of the network on the" in r2.stdout
    ev = json.loads(open(out / "eval.txt").read().strip().splitlines()[-1])
    print("cli probe: logged acc1 %.3f loss %.5f, --eval --resume acc1 %.3f loss %.5f"
          % (log[-1]["test_acc1"], log[-1]["test_loss"], ev["test_acc1"], ev["test_loss"]))
    assert ev["test_acc1"] == log[-1]["test_acc1"]
    assert abs(ev["test_loss"] - log[-1]["test_loss"]) <= 1e-5 * max(1.0, abs(log[-1]["test_loss"]))
    # --auto_resume (the default) of the frozen run: one more epoch, still frozen
    r3 = subprocess.run(base(out) + ["--epochs", "3", "--freeze_backbone", "1"], cwd=ROOT, env=env, capture_output=True,
                        text=True, timeout=900)
    assert r3.returncode == 0, r3.stdout[-3000:] + r3.stderr[-3000:]
    assert "froze blocks.0.attn.qkv.weight" in r3.stdout
    ck2 = torch.load(out / "checkpoint-2.pth", map_location="cpu", weights_only=False)
    assert all(torch.equal(v, ck0["model"][k]) for k, v in ck2["model"].items() if not k.startswith(("head.", "fc_norm.")))
    assert not torch.equal(ck2["model"]["head.weight"], ck1["model"]["head.weight"])
