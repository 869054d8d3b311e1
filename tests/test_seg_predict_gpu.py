"""-m gpu: memhip_seg_predict (csrc/seg_predict.hip) through mem_amd.ops.seg_predict.

The oracle is torch float64 on the CPU, written here as mmseg 0.30 writes it: per pass, F.interpolate(bilinear) of every view ->
preds += F.pad(view) and count_mat += 1 -> preds / count_mat -> softmax -> flip of the flipped pass -> mean over the passes ->
numpy's argmax (first occurrence: ties to the lowest class).  Exact cases must agree on every pixel.  Probabilities are held to
torch's own fp32 evaluation of the same restatement on the GPU: error(HIP) <= 2 x error(torch fp32) + 2^-20 x max |ref|; labels
must equal the float64 argmax wherever its top-2 margin is at least 1e-5 (about 50 times the fp32 error of a probability), and at
most 0.1 % of the pixels may fall below that margin.  Every figure is printed before it is asserted (run with -s)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

IGN = 255
FLOOR = 2.0 ** -20
MARGIN = 1e-5
LEFT_OUT = 1e-3


# ---------------------------------------------------------------- the restatement, the oracle, the call
def grid(canvas, crop, stride, flips=(0,)):
    from mem_amd.seg_infer import slide_windows
    return [(y1, x1, f) for f in flips for y1, x1 in slide_windows(canvas, crop, stride)]


def restate(logits, rects, window, canvas, align=False):
    """logits [V, B, C, h, w] on any device / dtype -> (P [B, C, H, W], L of the only pass in output coordinates or None)"""
    V, B, Cc, h, w = logits.shape
    (H, W), (hc, wc) = canvas, window
    passes = sorted({f for _, _, f in rects})
    total, last = None, None
    for f in passes:
        preds = logits.new_zeros((B, Cc, H, W))
        count = logits.new_zeros((1, 1, H, W))
        for v, (y1, x1, vf) in enumerate(rects):
            if vf != f:
                continue
            up = F.interpolate(logits[v], size=(hc, wc), mode="bilinear", align_corners=align)
            preds += F.pad(up, (x1, W - x1 - wc, y1, H - y1 - hc))
            count[:, :, y1:y1 + hc, x1:x1 + wc] += 1
        assert int((count == 0).sum()) == 0
        L = preds / count
        Pf = F.softmax(L, dim=1)
        if f:
            L, Pf = L.flip(3), Pf.flip(3)
        total = Pf if total is None else total + Pf
        last = L
    return total / len(passes), (last if len(passes) == 1 else None)


def oracle(logits, rects, window, canvas, align=False):
    """float64 on the CPU: P, pred (argmax of L with one pass, of P with two), the top-2 margin of P"""
    P, L = restate(logits.double().cpu(), rects, window, canvas, align)
    pred = np.argmax((L if L is not None else P).numpy(), axis=1).astype(np.uint8)
    top = torch.topk(P, 2, dim=1).values
    return P, pred, (top[:, 0] - top[:, 1]).numpy()


def confusion_of(pred, lab, Cc):
    lb = lab.numpy() if isinstance(lab, torch.Tensor) else lab
    v = (lb != IGN) & (lb < Cc)
    conf = np.zeros((Cc, Cc), np.int64)
    np.add.at(conf, (lb[v].astype(np.int64), pred[v].astype(np.int64)), 1)
    return conf


def make_labels(gen, B, Cc, H, W, p_ignore=0.2, n_bad=5):
    lab = torch.randint(0, Cc, (B, H, W), generator=gen)
    lab[torch.rand((B, H, W), generator=gen) < p_ignore] = IGN
    flat = lab.view(-1)
    for k in range(n_bad):
        flat[int(torch.randint(0, flat.numel(), (1,), generator=gen))] = Cc + (k % 2) * 100
    return lab.to(torch.uint8)


def hip(logits, rects, window, canvas, want_prob=True, labels=None, align=False):
    """-> (pred u8 numpy, prob f64 CPU or None, confusion numpy or None)"""
    from mem_amd import ops
    dev = torch.device("cuda")
    lg = logits if logits.is_cuda else logits.cuda()
    B, Cc = (lg.shape[1], lg.shape[2]) if lg.dim() == 5 else (lg.shape[0] // len(rects), lg.shape[1])
    H, W = canvas
    pred = torch.full((B, H, W), 254, dtype=torch.uint8, device=dev)
    prob = torch.full((B, Cc, H, W), float("nan"), device=dev) if want_prob else None
    conf = torch.zeros((Cc, Cc), dtype=torch.int64, device=dev) if labels is not None else None
    ops.seg_predict(lg, rects, window, canvas, pred=pred, prob=prob, labels=None if labels is None else labels.cuda(), confusion=conf,
                    align_corners=align)
    torch.cuda.synchronize()
    return pred.cpu().numpy(), (prob.cpu().double() if want_prob else None), (conf.cpu().numpy() if conf is not None else None)


def held(name, got, yard, ref, figures):
    e_got, e_yard = float((got - ref).abs().max()), float((yard - ref).abs().max())
    bound = 2.0 * e_yard + FLOOR * float(ref.abs().max())
    figures.append((name, e_got, e_yard, bound))
    return e_got <= bound


def check_tolerance(name, logits, rects, window, canvas, figures):
    """prob by the rule, pred on the margin, the left-out share under its cap"""
    ref_P, ref_pred, margin = oracle(logits, rects, window, canvas)
    yard = restate(logits.cuda(), rects, window, canvas)[0].cpu().double()
    pred, prob, _ = hip(logits, rects, window, canvas)
    ok = held(name, prob, yard, ref_P, figures)
    sure = margin >= MARGIN
    left_out = 1.0 - float(sure.mean())
    wrong = int((pred[sure] != ref_pred[sure]).sum())
    print("%s: prob hip=%.3e torch=%.3e bound=%.3e; left out %.4f %%, wrong on the margin %d, differing below it %d"
          % ((name,) + figures[-1][1:] + (100 * left_out, wrong, int((pred[~sure] != ref_pred[~sure]).sum()))))
    assert bool(torch.isfinite(prob).all())
    return ok and wrong == 0 and left_out <= LEFT_OUT


# ---------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("B,Cc", [(2, 5), (2, 11)])
def test_exact_labels_and_confusion_over_overlapping_windows(B, Cc):
    """ratio 4 and logits that are multiples of 1/8 in [-4, 4]: every weight is a multiple of 1/8, every sum of up to four views
    exact in fp32, and the counts 1, 2, 4 divide exactly: label and tie (to the lowest class) must agree with float64 on every
    pixel, and the matrix with it"""
    canvas, window = (48, 64), (32, 32)
    rects = grid(canvas, window, (16, 24))
    assert len(rects) == 6
    gen = torch.Generator().manual_seed(100 + Cc)
    z = torch.randint(-32, 33, (6, B, Cc, 8, 8), generator=gen).float() / 8
    z[:, :, :, :3, :2] = 0.5                            # all classes equal in every view: class 0
    z[:, :, :, 5:, 4:] = -4.0
    z[:, :, 1, 5:, 4:] = 4.0                            # classes 1 and 3 share the maximum: class 1
    z[:, :, 3, 5:, 4:] = 4.0
    z[:, 0, :, 0, 7] = -4.0
    z[:, 0, Cc - 1, 0, 7] = 4.0
    z[:, 0, 0, 0, 7] = 4.0                              # first and last class tie in a corner: class 0
    lab = make_labels(gen, B, Cc, *canvas)
    ref_P, ref_pred, margin = oracle(z, rects, window, canvas)
    pred, _, conf = hip(z, rects, window, canvas, want_prob=False, labels=lab)
    ties = int((margin == 0).sum())
    print("exact", (B, Cc), "pixels with an exact tie:", ties, "differing:", int((pred != ref_pred).sum()))
    assert ties > 100
    assert np.array_equal(pred, ref_pred)
    want = confusion_of(ref_pred, lab, Cc)
    assert 0 < want.sum() < lab.numel() and np.array_equal(conf, want)


# ---------------------------------------------------------------- 2. the labels of memhip_seg_confusion
@pytest.mark.parametrize("layout", ["nchw", "rows"])
@pytest.mark.parametrize("h,w,H,W", [(9, 17, 36, 68), (12, 16, 45, 70)])
def test_one_view_gives_the_confusion_kernels_labels_bit_for_bit(layout, h, w, H, W):
    from mem_amd.seg_loss import SegEvaluator
    B, Cc = 3, 11
    gen = torch.Generator().manual_seed(H + (layout == "rows"))
    if layout == "nchw":
        view = (torch.randn((B, Cc, h, w), generator=gen) * 3).cuda()
    else:
        view = (torch.randn((B * h * w, Cc + 3), generator=gen) * 3).cuda().view(B, h, w, Cc + 3)[..., :Cc].permute(0, 3, 1, 2)
    lab = make_labels(gen, B, Cc, H, W)
    ev = SegEvaluator(Cc)
    ev.update(view, lab.cuda())
    pred, _, conf = hip(view, [(0, 0, 0)], (H, W), (H, W), want_prob=False, labels=lab)
    assert np.array_equal(conf, ev.matrix.cpu().numpy())
    assert np.array_equal(confusion_of(pred, lab, Cc), conf)         # every counted pixel's label is the one that was counted
    assert np.array_equal(hip(view.unsqueeze(0), [(0, 0, 0)], (H, W), (H, W), want_prob=False)[0], pred)       # [V, B, C, h, w]


# ---------------------------------------------------------------- 3. tolerance, two passes
CASES = {
    "slide 48x64": ((48, 64), (32, 32), (16, 24), (8, 8), 11, 2),
    "slide 45x70": ((45, 70), (32, 40), (21, 27), (8, 10), 19, 2),
    "whole 48x64": ((48, 64), (48, 64), (48, 64), (12, 16), 5, 3),
}


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_two_passes_within_twice_torchs_own_error(case, seed):
    canvas, window, stride, hw, Cc, B = CASES[case]
    rects = grid(canvas, window, stride, flips=(0, 1))
    logits = torch.randn((len(rects), B, Cc) + hw, generator=torch.Generator().manual_seed(seed)) * 3
    figures = []
    assert check_tolerance("%s seed %d" % (case, seed), logits, rects, window, canvas, figures), figures


def test_flipped_pass_alone_and_align_corners():
    """one pass with flip = 1 is the mirrored whole image; align_corners=True reads the other tables"""
    canvas, hw, Cc, B = (45, 70), (12, 16), 7, 2
    logits = torch.randn((1, B, Cc) + hw, generator=torch.Generator().manual_seed(5)) * 3
    for rects, align in (([(0, 0, 1)], False), ([(0, 0, 0)], True)):
        ref_P, ref_pred, margin = oracle(logits, rects, canvas, canvas, align)
        yard = restate(logits.cuda(), rects, canvas, canvas, align)[0].cpu().double()
        pred, prob, _ = hip(logits, rects, canvas, canvas, align=align)
        figures = []
        ok = held((rects, align), prob, yard, ref_P, figures)
        sure = margin >= MARGIN
        print("flip / align", figures[-1], "left out", 1.0 - float(sure.mean()))
        assert ok and np.array_equal(pred[sure], ref_pred[sure]) and 1.0 - float(sure.mean()) <= LEFT_OUT


# ---------------------------------------------------------------- 4. every class-count instantiation
def test_every_class_instantiation_at_both_of_its_ends():
    """the kernel is instantiated for 8, 12, .. 32 padded classes: the smallest and largest C of each, one ragged canvas, both
    passes"""
    canvas, window, stride, hw, B = (37, 53), (20, 24), (17, 15), (5, 6), 2
    rects = grid(canvas, window, stride, flips=(0, 1))
    figures, failures = [], []
    for Cc in (2, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 32):
        logits = torch.randn((len(rects), B, Cc) + hw, generator=torch.Generator().manual_seed(1000 + Cc)) * 3
        if not check_tolerance("C=%d" % Cc, logits, rects, window, canvas, figures):
            failures.append(Cc)
    print("classes worst error/bound: %.3f" % max(f[1] / f[3] for f in figures))
    assert not failures, failures


# ---------------------------------------------------------------- 5. safety and determinism
@functools.lru_cache(maxsize=None)
def _slide_case():
    canvas, window, stride, hw, Cc, B = CASES["slide 45x70"]
    rects = grid(canvas, window, stride, flips=(0, 1))
    logits = (torch.randn((len(rects), B, Cc) + hw, generator=torch.Generator().manual_seed(9)) * 3).cuda()
    lab = make_labels(torch.Generator().manual_seed(10), B, Cc, *canvas)
    return canvas, window, rects, logits, lab, Cc, B


def test_two_calls_give_the_same_bits():
    canvas, window, rects, logits, lab, Cc, B = _slide_case()
    a = hip(logits, rects, window, canvas, labels=lab)
    b = hip(logits, rects, window, canvas, labels=lab)
    assert np.array_equal(a[0], b[0]) and a[1].numpy().tobytes() == b[1].numpy().tobytes() and np.array_equal(a[2], b[2])
    assert a[2].sum() > 0 and len(np.unique(a[0])) > 3


@pytest.mark.parametrize("canvas,offset", [((45, 70), 64), ((48, 64), 64), ((48, 64), 61)])
def test_guard_bands_stay_untouched_and_prob_is_fully_written(canvas, offset):
    """pred leaves as dwords (48 x 64 at an aligned address) or as bytes (a ragged width, an unaligned address); neither form
    writes outside the outputs, and a NaN-filled prob is overwritten everywhere"""
    from mem_amd import ops
    B, Cc, hw = 2, 5, (12, 16)
    H, W = canvas
    logits = (torch.randn((1, B, Cc) + hw, generator=torch.Generator().manual_seed(11)) * 3).cuda()
    n = B * H * W
    flat = torch.full((n + 2 * offset + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    pflat = torch.full((n * Cc + 128,), 12345.0, device="cuda")
    pflat[64: 64 + n * Cc] = float("nan")
    pred, prob = flat[offset: offset + n].view(B, H, W), pflat[64: 64 + n * Cc].view(B, Cc, H, W)
    assert ops.seg_predict_plan([(0, 0, 0)], B, Cc, hw, canvas, canvas, pred=pred.data_ptr()).pred_dwords == int(W % 4 == 0 and offset % 4 == 0)
    ops.seg_predict(logits, [(0, 0, 0)], canvas, canvas, pred=pred, prob=prob)
    torch.cuda.synchronize()
    assert bool((flat[:offset] == 0xAB).all()) and bool((flat[offset + n:] == 0xAB).all())
    assert bool((pflat[:64] == 12345.0).all()) and bool((pflat[64 + n * Cc:] == 12345.0).all())
    assert bool(torch.isfinite(prob).all()) and int(pred.max()) < Cc
    assert float((prob.sum(1) - 1.0).abs().max()) < 1e-5
    ref_P, ref_pred, margin = oracle(logits, [(0, 0, 0)], canvas, canvas)
    sure = margin >= MARGIN
    assert np.array_equal(pred.cpu().numpy()[sure], ref_pred[sure])


def test_confusion_is_added_to():
    from mem_amd import ops
    canvas, window, rects, logits, lab, Cc, B = _slide_case()
    once = hip(logits, rects, window, canvas, want_prob=False, labels=lab)[2]
    conf = torch.full((Cc, Cc), 7, dtype=torch.int64, device="cuda")
    for _ in range(2):
        ops.seg_predict(logits, rects, window, canvas, labels=lab.cuda(), confusion=conf)        # no pred: the matrix alone
    assert np.array_equal(conf.cpu().numpy(), 7 + 2 * once)


def test_sixty_four_thin_windows():
    canvas, window, hw, Cc = (8, 128), (8, 2), (4, 2), 4
    rects = [(0, x, 0) for x in range(0, 128, 2)]
    assert len(rects) == 64
    logits = torch.randn((64, 1, Cc) + hw, generator=torch.Generator().manual_seed(12)) * 3
    figures = []
    assert check_tolerance("64 views", logits, rects, window, canvas, figures), figures
    with pytest.raises(Exception, match="V=65"):
        hip(torch.zeros((65, 1, Cc) + hw), rects + [(0, 0, 0)], window, canvas)
