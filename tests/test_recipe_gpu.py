"""-m gpu: the finetuning recipe on the device -- memhip_mixup / mix_targets / ce_soft / ema_update against float64
restatements of their formulas, utils.ModelEma on a tiny ft_vit, and the recipe end to end (train_one_epoch, the stage-3
entrypoint in a child process)."""
import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U22 = 2.0 ** -22


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ mixup
def _mixup_case(B, C, H, W, lam, box):
    from mem_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + H)
    x0 = torch.randn(B, C, H, W, generator=g).cuda()
    x = x0.clone()
    ops.mixup(x, _dev(lam), _dev(box), lam, box)
    torch.cuda.synchronize()
    hh = torch.arange(H, device="cuda").view(1, 1, H, 1)
    ww = torch.arange(W, device="cuda").view(1, 1, 1, W)
    b = _dev(box).long()
    yl, yh, xl, xh = (b[:, k].view(B, 1, 1, 1) for k in range(4))
    has_box = ((yh > yl) & (xh > xl)).expand(B, C, H, W)
    inbox = (hh >= yl) & (hh < yh) & (ww >= xl) & (ww < xh) & has_box
    l64 = _dev(lam).double().view(B, 1, 1, 1)
    xi, xj = x0.double(), x0.flip(0).double()
    # box samples: exact copies everywhere
    want_box = torch.where(inbox, x0.flip(0), x0)
    assert torch.equal(x[has_box], want_box[has_box])
    # blend samples: three fp32 roundings with margin for one fused multiply-add
    blend = ~has_box
    ref = l64 * xi + (1 - l64) * xj
    err = (x.double() - ref).abs()
    bound = U22 * ((l64 * xi).abs() + ((1 - l64) * xj).abs())
    assert bool((err[blend] <= bound[blend]).all()), float((err - bound)[blend].max())
    ident = (_dev(lam) == 1).view(B, 1, 1, 1).expand(B, C, H, W) & blend
    assert torch.equal(x[ident], x0[ident])                         # lam = 1: untouched bit for bit
    return x, x0


@pytest.mark.parametrize("B", [2, 7, 256])
@pytest.mark.parametrize("chw", [(3, 224, 224), (2, 128, 128), (3, 30, 50)])
def test_mixup_kernel_against_float64(B, chw):
    C, H, W = chw
    r = np.random.RandomState(B + H)
    # per-sample parameters: blends (incl. lam = 0 and lam = 1) and boxes (incl. full-image, border and one-pixel boxes)
    lam = r.rand(B).astype(np.float32)
    box = np.zeros((B, 4), np.int32)
    lam[0] = 1.0
    lam[-1] = 0.0
    for i in range(1, B - 1):
        if i % 2:
            y0, x0 = r.randint(0, H), r.randint(0, W)
            box[i] = (y0, r.randint(y0 + 1, H + 1), x0, r.randint(x0 + 1, W + 1))
    if B > 4:
        box[1] = (0, H, 0, W)
        box[3] = (H - 1, H, W - 1, W)
        lam[2] = 1.0
    _mixup_case(B, C, H, W, lam, box)
    # whole-batch forms (mode='batch'): one blend, one box, one identity
    _mixup_case(B, C, H, W, np.full(B, 0.3, np.float32), np.zeros((B, 4), np.int32))
    _mixup_case(B, C, H, W, np.full(B, 0.6, np.float32), np.tile(np.array([[H // 4, H // 2 + 3, 1, W - 2]], np.int32), (B, 1)))
    x, x0 = _mixup_case(B, C, H, W, np.ones(B, np.float32), np.zeros((B, 4), np.int32))
    assert torch.equal(x, x0)


def test_mixup_unaligned_shape_takes_the_scalar_path():
    """C*H*W not a multiple of 4 (odd samples start off 16-byte alignment): same contract, 4-byte accesses."""
    lam = np.array([0.25, 0.5, 1.0, 0.0, 0.7], np.float32)
    box = np.array([[0, 0, 0, 0], [1, 3, 2, 7], [0, 0, 0, 0], [0, 0, 0, 0], [0, 5, 0, 7]], np.int32)
    _mixup_case(5, 3, 5, 7, lam, box)


# ------------------------------------------------------------------ soft targets
@pytest.mark.parametrize("B,V,s", [(8, 101, 0.1), (256, 1000, 0.1), (6, 2, 0.0), (5, 100, 0.3)])
def test_mix_targets_against_float64(B, V, s):
    from mem_amd import ops
    r = np.random.RandomState(V)
    lab = r.randint(0, V, B).astype(np.int64)
    lam = r.rand(B).astype(np.float32)
    lam[0] = 1.0
    out = torch.full((B, V), -7.0, device="cuda")
    ops.mix_targets(_dev(lab), _dev(lam), V, s, out)
    off = s / V
    on = 1.0 - s + off
    oh = np.full((B, V), off)
    oh[np.arange(B), lab] = on
    ref = lam.astype(np.float64)[:, None] * oh + (1 - lam.astype(np.float64))[:, None] * oh[::-1]
    got = out.double().cpu().numpy()
    assert np.abs(got - ref).max() <= 1e-7, np.abs(got - ref).max()
    assert np.abs(got.sum(1) - 1).max() <= 1e-6


def test_mix_targets_label_out_of_range_is_nan_not_a_fault():
    from mem_amd import ops
    B, V = 8, 101
    lab = torch.arange(B, device="cuda") * 3
    lab[2] = 2 ** 40
    lab[4] = -1
    out = torch.zeros(B, V, device="cuda")
    ops.mix_targets(lab, torch.full((B,), 0.4, device="cuda"), V, 0.1, out)
    torch.cuda.synchronize()
    bad = torch.zeros(B, dtype=torch.bool, device="cuda")
    bad[[2, 4, B - 1 - 2, B - 1 - 4]] = True                        # the row and its mixing partner
    assert torch.isnan(out[bad]).all() and torch.isfinite(out[~bad]).all()


# ------------------------------------------------------------------ soft-target / label-smoothing cross-entropy
SHAPES = [(256, 101), (37, 2), (64, 1000), (5, 100)]
# fp32 gradients, error measure max |g - g64| / max |g64| over the tensor (element-wise ratios are meaningless where softmax
# and target cancel): measured on an MI355X over these shapes and both target forms, worst 1.38e-7 (labels, (256, 101));
# the bound is 4 x that, far inside the 1e-4 ceiling.  test_ce_soft_against_float64 prints each figure.
F32_GRAD_MEASURED = 1.38e-7
F32_GRAD_BOUND = 4 * F32_GRAD_MEASURED


def _ce_inputs(M, V, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, V, generator=g) * 2.0).cuda().to(dtype)
    t = torch.rand(M, V, generator=g).cuda() ** 4
    t = t / t.sum(1, keepdim=True)
    y = torch.randint(0, V, (M,), generator=g).cuda()
    x[0, y[0]] = 30.0
    return x, t, y


def _ce_run(x, target=None, labels=None, smoothing=0.0, ld_pad=0):
    from mem_amd import ops
    M, V = x.shape
    if ld_pad:                                                        # a leading dimension beyond V
        buf = torch.zeros(M, V + ld_pad, dtype=x.dtype, device="cuda")
        buf[:, :V] = x
        x = buf[:, :V]
    dl = torch.empty(M, V, dtype=x.dtype, device="cuda")
    row_loss, row_ok, out2 = torch.zeros(M, device="cuda"), torch.zeros(M, dtype=torch.int32, device="cuda"), torch.zeros(2, device="cuda")
    ops.ce_soft(x, row_loss, row_ok, out2, target=target, labels=labels, smoothing=smoothing, grad_scale=1.0 / M, dlogits=dl)
    return out2, dl, row_loss


def _ce_ref(x, t64):
    """float64 on the same (already rounded) logits: loss, d(mean loss)/dx."""
    x64 = x.double().requires_grad_(True)
    loss = (-(t64 * torch.log_softmax(x64, -1)).sum(-1)).mean()
    loss.backward()
    return loss.detach(), x64.grad


def _smooth_onehot(y, V, s):
    t = torch.full((y.numel(), V), s / V, dtype=torch.float64, device="cuda")
    t[torch.arange(y.numel()), y] += 1.0 - s
    return t


@pytest.mark.parametrize("M,V", SHAPES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("form", ["dense", "labels"])
def test_ce_soft_against_float64(M, V, dtype, form):
    x, t, y = _ce_inputs(M, V, dtype, M + V)
    if form == "dense":
        out2, dl, _ = _ce_run(x, target=t, ld_pad=3)
        t64 = t.double()
        hard = t.argmax(-1)
    else:
        out2, dl, _ = _ce_run(x, labels=y, smoothing=0.1, ld_pad=3)
        t64 = _smooth_onehot(y, V, 0.1)
        hard = y
    loss, grad = _ce_ref(x, t64)
    print("ce_soft", form, dtype, (M, V), "loss", out2[0].item(), "ref", loss.item())
    torch.testing.assert_close(out2[0].double(), loss, rtol=1e-5, atol=1e-5)
    acc = (x.float().cpu().max(-1)[1] == hard.cpu()).float().mean().item()
    assert abs(out2[1].item() - acc) < 1e-6
    if dtype == torch.bfloat16:
        torch.testing.assert_close(dl.float(), grad.float().bfloat16().float(), rtol=2e-2, atol=1e-7)
    else:
        rel = ((dl.double() - grad).abs().max() / grad.abs().max()).item()
        print("ce_soft f32 grad: max |err| / max |ref| = %.3e" % rel)
        assert rel <= F32_GRAD_BOUND, rel


def test_ce_soft_labels_equal_cross_entropy_and_onehot_dense():
    """Form (b) with smoothing 0 == memhip_cross_entropy (V % 8 == 0) == form (a) with one-hot targets."""
    from mem_amd import ops
    M, V = 64, 1000
    x, _, y = _ce_inputs(M, V, torch.bfloat16, 5)
    lg = x.clone()
    row_loss, row_ok, o_ce = torch.zeros(M, device="cuda"), torch.zeros(M, dtype=torch.int32, device="cuda"), torch.zeros(2, device="cuda")
    ops.cross_entropy(lg, y, M, V, 1.0 / M, row_loss, row_ok, o_ce)
    o_b, dl_b, _ = _ce_run(x, labels=y, smoothing=0.0)
    o_a, dl_a, _ = _ce_run(x, target=_smooth_onehot(y, V, 0.0).float())
    for o, dl in ((o_b, dl_b), (o_a, dl_a)):
        torch.testing.assert_close(o[0], o_ce[0], rtol=1e-5, atol=1e-5)
        assert abs(o[1].item() - o_ce[1].item()) < 1e-6
        torch.testing.assert_close(dl.float(), lg.float(), rtol=2e-2, atol=1e-7)
    for Mv in ((37, 2), (256, 101)):                                  # (a) one-hot == (b), shapes memhip_cross_entropy cannot take
        x, _, y = _ce_inputs(*Mv, torch.float32, 6)
        o_b, dl_b, _ = _ce_run(x, labels=y, smoothing=0.0)
        o_a, dl_a, _ = _ce_run(x, target=_smooth_onehot(y, Mv[1], 0.0).float())
        torch.testing.assert_close(o_a, o_b, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(dl_a, dl_b, rtol=1e-5, atol=1e-7)


def test_ce_soft_in_place_and_label_out_of_range():
    M, V = 16, 101
    x, _, y = _ce_inputs(M, V, torch.float32, 9)
    from mem_amd import ops
    o1, dl, _ = _ce_run(x, labels=y, smoothing=0.1)
    xin = x.clone()
    row_loss, row_ok, o2 = torch.zeros(M, device="cuda"), torch.zeros(M, dtype=torch.int32, device="cuda"), torch.zeros(2, device="cuda")
    ops.ce_soft(xin, row_loss, row_ok, o2, labels=y, smoothing=0.1, grad_scale=1.0 / M, dlogits=xin)
    assert torch.equal(xin, dl) and torch.equal(o1, o2)
    y[3] = 2 ** 33
    y[5] = -2
    o3, dl3, rl = _ce_run(x, labels=y, smoothing=0.1)
    torch.cuda.synchronize()
    assert torch.isnan(rl[3]) and torch.isnan(rl[5]) and torch.isnan(o3[0]) and torch.isfinite(dl3).all()
    good = torch.ones(M, dtype=torch.bool, device="cuda"); good[3] = good[5] = False
    assert torch.isfinite(rl[good]).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_loss_modules_backward_scales_by_the_upstream_gradient(dtype):
    from mem_amd.loss import LabelSmoothingCrossEntropy, SoftTargetCrossEntropy
    M, V = 37, 101
    x, t, y = _ce_inputs(M, V, dtype, 12)
    for crit, tgt, t64 in ((SoftTargetCrossEntropy(), t, t.double()),
                           (LabelSmoothingCrossEntropy(0.1), y, _smooth_onehot(y, V, 0.1))):
        xa = x.clone().requires_grad_(True)
        loss = crit(xa, tgt)
        (loss * 3.5).backward()                                       # non-unit upstream gradient
        ref_loss, ref_grad = _ce_ref(x, t64)
        torch.testing.assert_close(loss.double(), ref_loss, rtol=1e-5, atol=1e-5)
        want = (ref_grad * 3.5).float()
        if dtype == torch.bfloat16:
            torch.testing.assert_close(xa.grad.float(), want.bfloat16().float(), rtol=3e-2, atol=1e-7)   # two bf16 roundings
        else:
            assert ((xa.grad.double() - want.double()).abs().max() / want.abs().max()).item() <= F32_GRAD_BOUND
        hard = tgt if tgt.dim() == 1 else tgt.argmax(-1)
        assert abs(crit.last_accuracy.item() - (x.float().argmax(-1) == hard).float().mean().item()) < 1e-6


# ------------------------------------------------------------------ EMA kernel
@pytest.mark.parametrize("n", [1, 1023, 2 ** 20 + 3])
@pytest.mark.parametrize("decay", [0.0, 0.5, 0.9999, 1.0])
def test_ema_update_against_float64(n, decay):
    from mem_amd import ops
    g = torch.Generator().manual_seed(n)
    e0, p = torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda()
    e = e0.clone()
    ops.ema_update(e, p, decay)
    ref = decay * e0.double() + (1 - decay) * p.double()
    bound = U22 * ((decay * e0.double()).abs() + ((1 - decay) * p.double()).abs())
    err = (e.double() - ref).abs()
    assert bool((err <= bound).all()), float((err - bound).max())
    if decay == 1.0:
        assert torch.equal(e, e0)


def test_ema_chained_updates_converge_geometrically():
    from mem_amd import ops
    decay, n = 0.9999, 4099
    e, p = torch.zeros(n, device="cuda"), torch.full((n,), 1.5, device="cuda")
    for _ in range(50):
        ops.ema_update(e, p, decay)
    want = 1.5 * (1 - decay ** 50)
    np.testing.assert_allclose(e.double().cpu().numpy(), want, rtol=1e-5)


# ------------------------------------------------------------------ ModelEma on a tiny ft_vit
def _tiny(num_classes=11, seed=0, **over):
    from mem_amd.modeling_finetune import ft_vit
    from oracle.gen_golden_ft import FT_A
    torch.manual_seed(seed)
    return ft_vit(**dict(FT_A, num_classes=num_classes, **over)).cuda()


def _optimizer(m, lr=2e-3):
    from mem_amd import optim_factory as OF
    depth = m.get_num_layers()
    assigner = OF.LayerDecayValueAssigner(list(0.75 ** (depth + 1 - i) for i in range(depth + 2)))

    class OA:
        opt = "adamw"; weight_decay = 0.05; opt_eps = 1e-8
    OA.lr = lr
    with contextlib.redirect_stdout(io.StringIO()):
        return OF.create_optimizer(OA(), m, skip_list=m.no_weight_decay(), get_num_layer=assigner.get_layer_id,
                                   get_layer_scale=assigner.get_scale)


def _quadrant_data(n_batches, B, classes=4, seed=3):
    """The separable task of test_pretrain_checkpoint_to_finetune_loop: the class decides which quadrant carries events."""
    g = torch.Generator().manual_seed(seed)
    data = []
    for _ in range(n_batches):
        y = torch.randint(0, classes, (B,), generator=g)
        x = torch.zeros(B, 3, 64, 96)
        for b in range(B):
            r, c = divmod(int(y[b]), 2)
            x[b, :, r * 32:(r + 1) * 32, c * 48:(c + 1) * 48] = (torch.rand(3, 32, 48, generator=g) < 0.3).float()
        data.append((x, y))
    return data


@pytest.mark.parametrize("engine_first", [False, True])
def test_model_ema_follows_the_float64_recurrence(engine_first):
    from mem_amd import utils as U
    m = _tiny(num_classes=4)
    if engine_first:
        m.engine
    state = torch.get_rng_state()
    ema = U.ModelEma(m, decay=0.9)
    assert torch.equal(torch.get_rng_state(), state)                    # the twin's init draws left the run's stream alone
    sd_m, sd_e = m.state_dict(), ema.ema.state_dict()
    assert list(sd_m) == list(sd_e) and all(torch.equal(sd_m[k], sd_e[k]) for k in sd_m)
    assert not ema.ema.training and ema.ema.engine is not m.engine
    opt, scaler, crit = _optimizer(m), U.NativeScalerWithGradNormCount(), torch.nn.CrossEntropyLoss()
    data = _quadrant_data(3, 8)
    m.train()
    for x, y in data:
        prev = {k: v.clone() for k, v in ema.ema.state_dict().items()}
        loss = crit(m(x.cuda()).float(), y.cuda())
        scaler(loss, opt, clip_grad=5.0, parameters=m.parameters())
        opt.zero_grad()
        ema.update(m)
        now, cur = ema.ema.state_dict(), m.state_dict()
        moved = 0
        for k in now:
            if not now[k].dtype.is_floating_point:
                assert torch.equal(now[k], cur[k])                       # integer buffers: copied
                continue
            a, b = 0.9 * prev[k].double(), (1 - 0.9) * cur[k].double()
            err = (now[k].double() - (a + b)).abs()
            assert bool((err <= U22 * (a.abs() + b.abs())).all()), k
            moved += int(not torch.equal(now[k], prev[k]))
        assert moved > 10
    with contextlib.redirect_stdout(io.StringIO()):
        from mem_amd import engine_for_finetuning as EF
        ev_m = EF.evaluate(data, m, torch.device("cuda"))
        ev_e = EF.evaluate(data, ema.ema, torch.device("cuda"))
    assert set(ev_e) == {"loss", "acc1", "acc5"} and np.isfinite(ev_e["loss"]) and ev_e["loss"] != ev_m["loss"]


def test_model_ema_checkpoint_round_trip(tmp_path):
    from mem_amd import utils as U
    m = _tiny(num_classes=4)
    ema = U.ModelEma(m, decay=0.5)
    opt, scaler = _optimizer(m), U.NativeScalerWithGradNormCount()
    x, y = _quadrant_data(1, 8)[0]
    m.train()
    scaler(torch.nn.CrossEntropyLoss()(m(x.cuda()).float(), y.cuda()), opt, clip_grad=5.0, parameters=m.parameters())
    ema.update(m)

    import argparse
    Args = argparse.Namespace(output_dir=str(tmp_path), auto_resume=True, resume="", model_ema=True, epochs=5, start_epoch=0)
    with contextlib.redirect_stdout(io.StringIO()):
        U.save_model(Args, 0, m, m, opt, scaler, model_ema=ema)
        ck = torch.load(os.path.join(tmp_path, "checkpoint-0.pth"), map_location="cpu", weights_only=False)
        m2 = _tiny(num_classes=4, seed=1)
        ema2 = U.ModelEma(m2, decay=0.5)
        opt2 = _optimizer(m2)
        U.auto_load_model(Args, m2, m2, opt2, scaler, model_ema=ema2)
    want, got = ema.ema.state_dict(), ema2.ema.state_dict()
    assert not torch.equal(want["head.weight"], m.state_dict()["head.weight"])      # the EMA is not the model
    assert all(torch.equal(want[k], got[k]) for k in want)
    assert all(torch.equal(v.cpu(), ck["model_ema"][k]) for k, v in want.items())
    assert all(torch.equal(v, m2.state_dict()[k]) for k, v in m.state_dict().items())
    # without an EMA the checkpoint has exactly the keys it had before this feature
    Args.output_dir = str(tmp_path / "plain"); os.makedirs(Args.output_dir)
    with contextlib.redirect_stdout(io.StringIO()):
        U.save_model(Args, 0, m, m, opt, scaler, model_ema=None)
    plain = torch.load(os.path.join(Args.output_dir, "checkpoint-0.pth"), map_location="cpu", weights_only=False)
    assert set(plain) == {"model", "optimizer", "epoch", "scaler", "args", "numerics", "drop_path_rng"} - \
        (set() if hasattr(m, "_dp_stream") else {"drop_path_rng"})
    assert set(ck) == set(plain) | {"model_ema"}


# ------------------------------------------------------------------ end to end
def test_recipe_train_one_epoch_loss_goes_down():
    """Mixup(0.8 / 1.0, prob 1, smoothing 0.1) + SoftTargetCrossEntropy + ModelEma + update_freq 2 on the separable quadrant
    task.  The soft-target loss has a floor well above zero (the entropy of the mixed, smoothed targets: about 0.5 nat for a
    uniform lam between two classes), so the acceptance is 'the loss goes down' from its start near ln 4, not the plain
    loop's factor 0.5."""
    from mem_amd import engine_for_finetuning as EF
    from mem_amd import utils as U
    from mem_amd.loss import SoftTargetCrossEntropy
    from mem_amd.mixup import Mixup
    m = _tiny(num_classes=4, drop_path_rate=0.1)
    ema = U.ModelEma(m, decay=0.9)
    opt, scaler = _optimizer(m), U.NativeScalerWithGradNormCount()
    data = _quadrant_data(6, 16)
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, label_smoothing=0.1, num_classes=4, rng=np.random.RandomState(0))
    crit = SoftTargetCrossEntropy()
    steps = len(data) // 2
    lr_sched = U.cosine_scheduler(2e-3, 1e-5, 8, steps, warmup_epochs=1)
    first = last = None
    with contextlib.redirect_stdout(io.StringIO()):
        for ep in range(8):
            st = EF.train_one_epoch(None, m, crit, data, opt, torch.device("cuda"), ep, scaler, max_norm=5.0, model_ema=ema,
                                    mixup_fn=mix, start_steps=ep * steps, lr_schedule_values=lr_sched,
                                    num_training_steps_per_epoch=steps, update_freq=2)
            first = st if first is None else first
            last = st
        ev = EF.evaluate(data, m, torch.device("cuda"))
        ev_ema = EF.evaluate(data, ema.ema, torch.device("cuda"))
    print("recipe loop: loss %.4f -> %.4f, acc1 %.1f, ema acc1 %.1f" % (first["loss"], last["loss"], ev["acc1"], ev_ema["acc1"]))
    assert np.isfinite(last["loss"]) and last["loss"] < first["loss"], (first["loss"], last["loss"])
    assert first["loss"] < 1.1 * np.log(4) + 0.1
    assert not torch.equal(ema.ema.state_dict()["head.weight"], m.state_dict()["head.weight"])


def test_soft_target_arm_equals_cross_entropy_arm_when_nothing_is_mixed():
    """Mixup(prob=0, label_smoothing=0) + SoftTargetCrossEntropy against nn.CrossEntropyLoss: same weights, same batch, no
    drop path, no dropout -- the two arms differ in the loss kernel only."""
    from mem_amd.loss import SoftTargetCrossEntropy
    from mem_amd.mixup import Mixup
    m = _tiny(num_classes=11)
    x, y = _quadrant_data(1, 16)[0]
    x, y = x.cuda(), y.cuda()
    m.train()
    eng = m.engine
    loss_a = torch.nn.CrossEntropyLoss()(m(x).float(), y)
    loss_a.backward()
    ga = eng.flat_g.clone()
    eng.flat_g.zero_()
    xm, soft = Mixup(prob=0.0, label_smoothing=0.0, num_classes=11)(x.clone(), y)
    assert torch.equal(xm, x) and torch.equal(soft.argmax(-1), y) and bool((soft.sum(-1) == 1).all())
    loss_b = SoftTargetCrossEntropy()(m(xm), soft)
    loss_b.backward()
    gb = eng.flat_g.clone()
    torch.testing.assert_close(loss_b, loss_a, rtol=1e-5, atol=0)
    worst = 0.0
    for name, (o, k) in eng.segs.items():
        if name.endswith("qkvbias3"):
            continue
        rel = ((gb[o:o + k] - ga[o:o + k]).norm() / (ga[o:o + k].norm() + 1e-12)).item()
        worst = max(worst, rel)
        assert rel <= 3e-2, (name, rel)
    print("soft-target vs CE arm: worst per-tensor rel-L2 of the gradients = %.3e" % worst)


def test_cli_two_epochs_then_eval_resume(tmp_path):
    """python -m mem_amd.run_class_finetuning in a fresh child process: 2 epochs on synthetic streams with the full recipe,
    checkpoints carry model_ema, and --eval --resume reproduces the logged accuracy."""
    from conftest import ROOT
    out = tmp_path / "run"
    out.mkdir()
    base = [sys.executable, "-m", "mem_amd.run_class_finetuning", "--expweek", "t", "--data_path", "synthetic", "--nb_classes", "4",
            "--input_H", "64", "--input_W", "96", "--batch_size", "8", "--synthetic_samples", "32", "--num_workers", "0",
            "--transformer_depth", "2", "--transformer_emb", "128", "--transformer_heads", "2", "--rand_aug", "0",
            "--slice_max_evs", "5000", "--output_dir", str(out), "--layer_decay", "0.75", "--lr", "1e-3"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(base + ["--epochs", "2", "--warmup_epochs", "0", "--save_ckpt_freq", "1", "--update_freq", "2",
                               "--mixup_prob", "1.0", "--model_ema_decay", "0.9"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Mixup is activated!" in r.stdout and "SoftTargetCrossEntropy" in r.stdout and "Using EMA" in r.stdout
    log = [json.loads(l) for l in open(out / "log.txt")]
    assert len(log) == 2 and all(np.isfinite(e["train_loss"]) and "test_acc1" in e and "ema_test_acc1" in e for e in log)
    ck = torch.load(out / "checkpoint-1.pth", map_location="cpu", weights_only=False)
    assert "model_ema" in ck and list(ck["model_ema"]) == list(ck["model"])
    assert not torch.equal(ck["model_ema"]["head.weight"], ck["model"]["head.weight"])
    assert (out / "checkpoint-best.pth").exists()
    r2 = subprocess.run(base + ["--eval", "--resume", str(out / "checkpoint-1.pth")], cwd=ROOT, env=env, capture_output=True,
                        text=True, timeout=900)
    assert r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-3000:]
    ev = json.loads(open(out / "eval.txt").read().strip().splitlines()[-1])
    print("cli: logged acc1 %.3f loss %.5f, --eval --resume acc1 %.3f loss %.5f"
          % (log[-1]["test_acc1"], log[-1]["test_loss"], ev["test_acc1"], ev["test_loss"]))
    assert ev["test_acc1"] == log[-1]["test_acc1"]
    assert abs(ev["test_loss"] - log[-1]["test_loss"]) <= 1e-5 * max(1.0, abs(log[-1]["test_loss"]))
