"""-m gpu: the fused resize + cross-entropy and the confusion kernel (csrc/seg_loss.hip) through mem_amd.seg_loss.

The oracle is torch float64 on the CPU, written here: F.interpolate(bilinear) -> F.cross_entropy(reduction='sum') * loss_weight
/ N and its autograd gradient, numpy's argmax (first occurrence: ties to the lowest class) for the counts and the confusion
matrix.  Counts and matrices must be EXACT.  Loss and gradient are held to torch's own fp32 evaluation of the same expression
on the same inputs on the GPU: error(HIP) <= 2 x error(torch fp32) + 2^-20 x the largest magnitude of the float64 result --
the factor because both sides evaluate the same fp32 chain in different orders, the floor because torch's error is sometimes
exactly zero.  Every figure is printed before it is asserted (run with -s to see them)."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

IGN = 255
FLOOR = 2.0 ** -20


# ---------------------------------------------------------------- inputs, oracle, the three evaluations
def make_view(leaf, layout, B, Cc, h, w):
    """the logical [B, C, h, w] logits on a leaf: NCHW as it is, or the first C columns of pixel rows [B h w, C + 3]"""
    if layout == "nchw":
        return leaf
    return leaf.view(B, h, w, Cc + 3)[..., :Cc].permute(0, 3, 1, 2)


def make_leaf(gen, layout, B, Cc, h, w, scale=3.0):
    shape = (B, Cc, h, w) if layout == "nchw" else (B * h * w, Cc + 3)
    return (torch.randn(shape, generator=gen) * scale).float()


def make_labels(gen, B, Cc, H, W, p_ignore=0.2, n_bad=3):
    lab = torch.randint(0, Cc, (B, H, W), generator=gen)
    lab[torch.rand((B, H, W), generator=gen) < p_ignore] = IGN
    flat = lab.view(-1)
    for k in range(min(n_bad, flat.numel() // 4)):
        flat[int(torch.randint(0, flat.numel(), (1,), generator=gen))] = Cc + (k % 2) * 100       # C and C + 100: both < 255
    return lab.to(torch.uint8)


def expression(leaf, lab_long, layout, B, Cc, h, w, align, loss_weight, avg_non_ignore):
    """the torch expression on any device / dtype: (loss, up, valid, bad); labels >= C count as ignored"""
    up = F.interpolate(make_view(leaf, layout, B, Cc, h, w), size=tuple(lab_long.shape[1:]), mode="bilinear", align_corners=align)
    counted = lab_long != IGN
    valid = counted & (lab_long < Cc)
    tgt = torch.where(valid, lab_long, torch.full_like(lab_long, -100))
    s = F.cross_entropy(up, tgt, ignore_index=-100, reduction="sum")
    n = max(int(valid.sum()), 1) if avg_non_ignore else lab_long.numel()
    return s * (loss_weight / n), up, valid, counted & ~valid


def oracle(leaf, lab, layout, B, Cc, h, w, align, loss_weight=1.0, avg_non_ignore=False):
    """float64 on the CPU: loss, d loss / d leaf, (n_valid, n_correct, n_bad), confusion matrix"""
    l64 = leaf.detach().double().cpu().requires_grad_()
    lab_long = lab.cpu().long()
    loss, up, valid, bad = expression(l64, lab_long, layout, B, Cc, h, w, align, loss_weight, avg_non_ignore)
    loss.backward()
    pred = np.argmax(up.detach().numpy(), axis=1)
    v, lb = valid.numpy(), lab_long.numpy()
    conf = np.zeros((Cc, Cc), np.int64)
    np.add.at(conf, (lb[v], pred[v]), 1)
    stats = (int(v.sum()), int((pred[v] == lb[v]).sum()), int(bad.sum()))
    return loss.detach(), l64.grad, stats, conf


def torch_fp32(leaf, lab, layout, B, Cc, h, w, align, loss_weight=1.0, avg_non_ignore=False):
    l32 = leaf.detach().cuda().requires_grad_()
    loss = expression(l32, lab.cuda().long(), layout, B, Cc, h, w, align, loss_weight, avg_non_ignore)[0]
    loss.backward()
    return loss.detach().cpu().double(), l32.grad.cpu().double()


def hip(leaf, lab, layout, B, Cc, h, w, align, loss_weight=1.0, avg_non_ignore=False):
    from mem_amd.seg_loss import SegCrossEntropy
    mod = SegCrossEntropy(IGN, align, loss_weight, avg_non_ignore)
    lh = leaf.detach().cuda().requires_grad_()
    loss = mod(make_view(lh, layout, B, Cc, h, w), lab.cuda())
    loss.backward()
    stats = tuple(int(mod.last_stats[k]) for k in ("n_valid", "n_correct", "n_bad"))
    return loss.detach().cpu().double(), lh.grad.cpu().double(), stats, mod


def held(name, got, yard, ref, figures):
    """error(got) <= 2 error(yard) + 2^-20 max |ref|; the three figures are appended to `figures`"""
    e_got, e_yard = float((got - ref).abs().max()), float((yard - ref).abs().max())
    bound = 2.0 * e_yard + FLOOR * float(ref.abs().max())
    figures.append((name, e_got, e_yard, bound))
    return e_got <= bound


# ---------------------------------------------------------------- exact
@pytest.mark.parametrize("B,Cc,h,w", [(2, 5, 3, 5), (2, 11, 9, 17)])
def test_counts_and_confusion_are_exact(B, Cc, h, w):
    """ratio 4, logits multiples of 1/8 in [-4, 4]: every weight is a multiple of 1/8 and every interpolated logit exact in
    fp32, so argmax and ties (to the lowest class) must agree with float64 on every pixel"""
    from mem_amd.seg_loss import SegEvaluator
    H, W = 4 * h, 4 * w
    gen = torch.Generator().manual_seed(100 + Cc)
    z = torch.randint(-32, 33, (B, Cc, h, w), generator=gen).float() / 8
    z[:, :, : (h + 1) // 2, :2] = 0.5                  # all classes equal: the argmax is class 0
    z[:, 1, h // 2:, w // 2:] = 4.0                    # classes 1 and 3 share the maximum: class 1
    z[:, 3, h // 2:, w // 2:] = 4.0
    z[0, Cc - 1, 0, w - 1] = 4.0
    z[0, 0, 0, w - 1] = 4.0                            # first and last class tie in a corner
    lab = make_labels(gen, B, Cc, H, W, n_bad=5)
    _, _, stats, conf = oracle(z, lab, "nchw", B, Cc, h, w, False)
    got = hip(z, lab, "nchw", B, Cc, h, w, False)
    print("exact", (B, Cc, h, w), "oracle", stats, "hip", got[2])
    assert stats[2] >= 1 and stats[0] > 0 and stats[0] - stats[1] > 0
    assert got[2] == stats
    ev = SegEvaluator(Cc)
    ev.update(z.cuda(), lab.cuda())
    assert np.array_equal(ev.matrix.cpu().numpy(), conf)
    assert int(ev.matrix.sum()) == stats[0] and int(ev.matrix.diag().sum()) == stats[1]
    # mmseg's int64 [B, 1, H, W] labels give the same
    ev.reset()
    ev.update(z.cuda(), lab.cuda().long().unsqueeze(1))
    assert np.array_equal(ev.matrix.cpu().numpy(), conf)


# ---------------------------------------------------------------- tolerance
SHAPES = [(1, 1, 1, 1), (1, 1, 4, 4), (2, 3, 2, 3), (3, 5, 7, 11), (7, 7, 9, 13), (8, 8, 32, 32), (9, 17, 36, 68), (17, 9, 68, 36)]


@pytest.mark.parametrize("h,w,H,W", SHAPES)
def test_loss_and_gradient_within_twice_torchs_own_error(h, w, H, W):
    figures, failures = [], []
    for Cc, B, align, layout, avg in itertools.product((2, 11, 19, 32), (1, 3), (False, True), ("nchw", "rows"), (False, True)):
        gen = torch.Generator().manual_seed(hash((h, w, H, W, Cc, B, align)) % (2 ** 31))
        leaf = make_leaf(gen, layout, B, Cc, h, w)
        lab = make_labels(gen, B, Cc, H, W)
        case = (Cc, B, int(align), layout, int(avg))
        ref_loss, ref_grad, ref_stats, _ = oracle(leaf, lab, layout, B, Cc, h, w, align, 1.0, avg)
        y_loss, y_grad = torch_fp32(leaf, lab, layout, B, Cc, h, w, align, 1.0, avg)
        g_loss, g_grad, g_stats, _ = hip(leaf, lab, layout, B, Cc, h, w, align, 1.0, avg)
        ok = held(case + ("loss",), g_loss, y_loss, ref_loss, figures)
        ok &= held(case + ("dz",), g_grad, y_grad, ref_grad.double(), figures)
        ok &= bool(torch.isfinite(g_grad).all()) and g_stats[0] == ref_stats[0] and g_stats[2] == ref_stats[2]
        if not ok:
            failures.append(case)
    worst = {}
    for name, e_got, e_yard, bound in figures:
        r = e_got / bound if bound > 0 else 0.0
        if r >= worst.get(name[-1], (-1.0,))[0]:
            worst[name[-1]] = (r, name, e_got, e_yard, bound)
    for k, v in worst.items():
        print("tolerance %dx%d->%dx%d worst %s: error/bound=%.3f case=%s hip=%.3e torch=%.3e bound=%.3e" % ((h, w, H, W, k) + v))
    assert not failures, failures


def test_every_channel_instantiation_at_both_of_its_ends():
    """the training kernel is instantiated for 8, 12, .. 32 channels: the smallest and largest C of each, one ragged shape"""
    h, w, H, W, B = 9, 17, 36, 68, 2
    figures, failures = [], []
    for Cc in (3, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 31):
        gen = torch.Generator().manual_seed(1000 + Cc)
        leaf, lab = make_leaf(gen, "nchw", B, Cc, h, w), make_labels(gen, B, Cc, H, W)
        ref = oracle(leaf, lab, "nchw", B, Cc, h, w, False)
        yard = torch_fp32(leaf, lab, "nchw", B, Cc, h, w, False)
        got = hip(leaf, lab, "nchw", B, Cc, h, w, False)
        ok = held((Cc, "loss"), got[0], yard[0], ref[0], figures) & held((Cc, "dz"), got[1], yard[1], ref[1], figures)
        if not (ok and got[2][0] == ref[2][0] and got[2][2] == ref[2][2]):
            failures.append(Cc)
    print("channels worst error/bound: %.3f" % max(f[1] / f[3] for f in figures))
    assert not failures, failures


def test_two_calls_give_the_same_bits():
    B, Cc, h, w, H, W = 3, 11, 9, 17, 36, 68
    gen = torch.Generator().manual_seed(7)
    leaf, lab = make_leaf(gen, "nchw", B, Cc, h, w), make_labels(gen, B, Cc, H, W)
    a = hip(leaf, lab, "nchw", B, Cc, h, w, False)
    b = hip(leaf, lab, "nchw", B, Cc, h, w, False)
    assert a[0].numpy().tobytes() == b[0].numpy().tobytes()
    assert torch.equal(a[1], b[1]) and a[2] == b[2]
    assert float(a[1].abs().max()) > 0


# ---------------------------------------------------------------- edges
@pytest.mark.parametrize("avg", [False, True])
def test_all_labels_ignored_gives_zero_not_nan(avg):
    B, Cc, h, w, H, W = 2, 11, 9, 17, 36, 68
    leaf = make_leaf(torch.Generator().manual_seed(3), "nchw", B, Cc, h, w)
    lab = torch.full((B, H, W), IGN, dtype=torch.uint8)
    loss, grad, stats, mod = hip(leaf, lab, "nchw", B, Cc, h, w, False, 1.0, avg)
    assert float(loss) == 0.0 and stats == (0, 0, 0)
    assert torch.equal(grad, torch.zeros_like(grad))
    assert float(mod.acc_seg()) == 0.0


@pytest.mark.parametrize("corner", [(0, 0), (0, 67), (35, 0), (35, 67)])
def test_one_valid_pixel_in_a_corner(corner):
    B, Cc, h, w, H, W = 2, 11, 9, 17, 36, 68
    leaf = make_leaf(torch.Generator().manual_seed(4), "nchw", B, Cc, h, w)
    lab = torch.full((B, H, W), IGN, dtype=torch.uint8)
    lab[1, corner[0], corner[1]] = 4
    for avg in (False, True):
        ref = oracle(leaf, lab, "nchw", B, Cc, h, w, False, 1.0, avg)
        yard = torch_fp32(leaf, lab, "nchw", B, Cc, h, w, False, 1.0, avg)
        got = hip(leaf, lab, "nchw", B, Cc, h, w, False, 1.0, avg)
        figures = []
        ok = held("loss", got[0], yard[0], ref[0], figures) & held("dz", got[1], yard[1], ref[1], figures)
        print("corner", corner, avg, figures)
        assert ok and got[2] == ref[2] and got[2][0] == 1
        assert int((got[1] != 0).sum()) == Cc                       # a corner output reads one logit per class


def test_a_logit_of_1e4_stays_finite_and_matches():
    B, Cc, h, w, H, W = 1, 11, 9, 17, 36, 68
    gen = torch.Generator().manual_seed(5)
    leaf, lab = make_leaf(gen, "nchw", B, Cc, h, w), make_labels(gen, B, Cc, H, W)
    leaf[0, 3, 4, 8] = 1e4
    ref = oracle(leaf, lab, "nchw", B, Cc, h, w, False)
    yard = torch_fp32(leaf, lab, "nchw", B, Cc, h, w, False)
    got = hip(leaf, lab, "nchw", B, Cc, h, w, False)
    figures = []
    ok = held("loss", got[0], yard[0], ref[0], figures) & held("dz", got[1], yard[1], ref[1], figures)
    print("1e4", figures)
    assert bool(torch.isfinite(got[0])) and bool(torch.isfinite(got[1]).all())
    assert ok and got[2] == ref[2]


# ---------------------------------------------------------------- bounds
@pytest.mark.parametrize("h,w,H,W", [(3, 5, 7, 11), (7, 7, 9, 13), (9, 17, 36, 68), (17, 9, 68, 36)])
def test_nothing_is_written_outside_dz_workspace_and_stats(h, w, H, W):
    from mem_amd import ops
    B, Cc = 3, 11
    gen = torch.Generator().manual_seed(6)
    z, lab = make_leaf(gen, "nchw", B, Cc, h, w).cuda(), make_labels(gen, B, Cc, H, W).cuda()
    need = int(ops.seg_plan(B, Cc, h, w, H, W).ws_bytes)
    pad = 256
    big_dz = torch.full((pad + z.numel() + pad,), 777.0, device="cuda")
    big_ws = torch.full((pad + need + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    big_loss = torch.full((pad + 3 + pad,), 777.0, device="cuda")
    big_stats = torch.full((pad + 3 + pad,), -777, dtype=torch.int64, device="cuda")
    dz = big_dz[pad:pad + z.numel()].view(B, Cc, h, w)
    ops.seg_ce(z, lab, dz, big_loss[pad:pad + 3], big_stats[pad:pad + 3], big_ws[pad:pad + need])
    torch.cuda.synchronize()
    for big, n in ((big_dz, z.numel()), (big_loss, 3)):
        assert bool((big[:pad] == 777.0).all()) and bool((big[pad + n:] == 777.0).all())
    assert bool((big_ws[:pad] == 0xA5).all()) and bool((big_ws[pad + need:] == 0xA5).all())
    assert bool((big_stats[:pad] == -777).all()) and bool((big_stats[pad + 3:] == -777).all())
    # and what is inside was written: every dz element, the stats, the loss
    ref = oracle(z.cpu(), lab.cpu(), "nchw", B, Cc, h, w, False)
    assert tuple(int(v) for v in big_stats[pad:pad + 3]) == ref[2]
    assert not bool((dz == 777.0).any())
    scale = float(big_loss[pad + 1])
    assert scale == pytest.approx(1.0 / (B * H * W), rel=1e-6)
    # (a plausibility check that dz holds the gradient -- 1e-5 of the largest value is ~100 fp32 roundings, more than the
    # chain has; the tolerance proper is test_loss_and_gradient_within_twice_torchs_own_error)
    assert float((dz.cpu().double() * scale - ref[1]).abs().max()) <= 1e-5 * float(ref[1].abs().max())
    # the confusion matrix, too, sits between sentinels
    big_conf = torch.full((pad + Cc * Cc + pad,), 0, dtype=torch.int64, device="cuda")
    big_conf[:pad] = -777
    big_conf[pad + Cc * Cc:] = -777
    ops.seg_confusion(z, lab, big_conf[pad:pad + Cc * Cc].view(Cc, Cc))
    assert bool((big_conf[:pad] == -777).all()) and bool((big_conf[pad + Cc * Cc:] == -777).all())
    assert np.array_equal(big_conf[pad:pad + Cc * Cc].view(Cc, Cc).cpu().numpy(), ref[3])


# ---------------------------------------------------------------- autograd through a torch head
def test_a_torch_head_trains_through_the_loss():
    from mem_amd.seg_loss import SegCrossEntropy
    B, Cin, Cc, h, w, H, W = 2, 8, 11, 9, 17, 36, 68
    gen = torch.Generator().manual_seed(8)
    x = torch.randn((B, Cin, h, w), generator=gen)
    lab = make_labels(gen, B, Cc, H, W)
    torch.manual_seed(9)
    head = torch.nn.Conv2d(Cin, Cc, 1)

    def grads(device, dtype, loss_fn):
        m = torch.nn.Conv2d(Cin, Cc, 1).to(device=device, dtype=dtype)
        m.load_state_dict({k: v.to(device=device, dtype=dtype) for k, v in head.state_dict().items()})
        loss = loss_fn(m(x.to(device=device, dtype=dtype)))
        loss.backward()
        return loss.detach().cpu().double(), m.weight.grad.cpu().double(), m.bias.grad.cpu().double()

    def torch_loss(z):
        return expression(z, lab.to(z.device).long(), "nchw", B, Cc, h, w, False, 0.4, False)[0]

    mod = SegCrossEntropy(loss_weight=0.4)
    ref = grads("cpu", torch.float64, torch_loss)
    yard = grads("cuda", torch.float32, torch_loss)
    got = grads("cuda", torch.float32, lambda z: mod(z, lab.cuda().long().unsqueeze(1)))
    figures = []
    ok = all([held(n, g, y, r, figures) for n, g, y, r in zip(("loss", "dweight", "dbias"), got, yard, ref)])
    print("autograd", figures)
    assert ok
    # acc_seg of the last call: the oracle's counts on the logits that call saw
    with torch.no_grad():
        z32 = F.conv2d(x.cuda(), head.weight.detach().cuda(), head.bias.detach().cuda())
    stats = oracle(z32, lab, "nchw", B, Cc, h, w, False)[2]
    assert float(mod.acc_seg()) == 100.0 * stats[1] / stats[0]
    with pytest.raises(Exception, match="labels >= 11"):
        SegCrossEntropy(check_labels=True)(torch.zeros((B, Cc, h, w), device="cuda"), lab.cuda())


# ---------------------------------------------------------------- evaluator
def test_evaluator_accumulates_and_both_layouts_agree():
    from mem_amd.seg_loss import SegEvaluator, metrics_from_confusion
    B, Cc, h, w, H, W = 3, 11, 9, 17, 36, 68
    gen = torch.Generator().manual_seed(10)
    ev, ev_rows, total = SegEvaluator(Cc), SegEvaluator(Cc), np.zeros((Cc, Cc), np.int64)
    for _ in range(2):
        rows = make_leaf(gen, "rows", B, Cc, h, w)
        lab = make_labels(gen, B, Cc, H, W)
        view = make_view(rows, "rows", B, Cc, h, w)
        total += oracle(rows, lab, "rows", B, Cc, h, w, False)[3]
        ev.update(view.contiguous().cuda(), lab.cuda())
        ev_rows.update(make_view(rows.cuda(), "rows", B, Cc, h, w), lab.cuda())
    # (a random fp32 input has no ties and no argmax decided by the last bit at these sizes: the matrices are exact)
    assert np.array_equal(ev.matrix.cpu().numpy(), total)
    assert torch.equal(ev.matrix, ev_rows.matrix)
    got, want = ev.compute(), metrics_from_confusion(torch.from_numpy(total))
    inter, label, pred = np.diag(total).astype(float), total.sum(1).astype(float), total.sum(0).astype(float)
    assert got["aAcc"] == pytest.approx(inter.sum() / label.sum())
    assert got["mIoU"] == pytest.approx(np.nanmean(inter / (label + pred - inter))) and got["mIoU"] == want["mIoU"]
    assert got["mAcc"] == pytest.approx(np.nanmean(inter / label))
    ev.reset()
    assert int(ev.matrix.sum()) == 0
