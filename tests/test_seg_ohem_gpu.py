"""-m gpu: class weights and OHEM pixel sampling inside the fused segmentation loss (csrc/seg_ohem.hip, csrc/seg_loss.hip)
through mem_amd.ops and mem_amd.seg_loss.

The oracle is torch float64 on the CPU, written here from the definition (interpolate -> log-softmax -> sort).  The selection
is held EXACTLY (bit for bit against torch.sort of the same fp32 keys); keys, loss and gradient are held to the project's rule
of tests/test_seg_loss_gpu.py: error(HIP) <= 2 x error(torch fp32 of the same expression on the GPU) + 2^-20 x max |float64
result|.  For loss and gradient the HIP arm's own keep mask is handed to the oracle and to the yardstick, so that a borderline
pixel cannot hide in the tolerance; the mask itself is held against float64's in a test of its own, where a pixel may differ
only when its float64 key lies within a relative 2^-16 of the float64 threshold, and at most 2 per case.  Every figure is
printed before it is asserted (run with -s to see them)."""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

IGN = 255
FLOOR = 2.0 ** -20
SHAPES = [(3, 5, 7, 11), (9, 17, 36, 68), (8, 8, 32, 32)]
CLASSES = (2, 11, 19, 32)


# ---------------------------------------------------------------- inputs (the recipe of tests/test_seg_loss_gpu.py)
def make_view(leaf, layout, B, Cc, h, w):
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
        flat[int(torch.randint(0, flat.numel(), (1,), generator=gen))] = Cc + (k % 2) * 100
    return lab.to(torch.uint8)


def make_weights(gen, Cc):
    cw = torch.rand(Cc, generator=gen) * 3.0
    cw[int(torch.randint(0, Cc, (1,), generator=gen))] = 0.0
    return cw.float()


# ---------------------------------------------------------------- the definition, on any device / dtype
def pieces(view, lab_long, cw, align):
    """(nll, prob of the label, cw[label], valid, bad, up) of the resized logits; cw None: ones"""
    Cc = view.shape[1]
    up = F.interpolate(view, size=tuple(lab_long.shape[1:]), mode="bilinear", align_corners=align)
    counted = lab_long != IGN
    valid = counted & (lab_long < Cc)
    tgt = torch.where(valid, lab_long, torch.zeros_like(lab_long))
    logp = F.log_softmax(up, 1).gather(1, tgt[:, None])[:, 0]
    wl = torch.ones_like(logp) if cw is None else cw.to(logp)[tgt]
    return -logp, logp.exp(), wl, valid, counted & ~valid, up


def keys_of(view, lab_long, cw, align, mode):
    """the sampler's key map, -1 where the pixel is not valid (mode 1: prob of the label, mode 2: cw * nll)"""
    nll, prob, wl, valid, _, _ = pieces(view, lab_long, cw, align)
    key = prob if mode == 1 else wl * nll
    return torch.where(valid, key, torch.full_like(key, -1.0)), valid


def select(keys, mode, K, T):
    """(threshold, keep mask) of the definition on a key map of any dtype: sort-based"""
    valid = keys >= 0
    n = int(valid.sum())
    if mode == 1:
        if n == 0:
            return keys.new_tensor(-math.inf), torch.zeros_like(valid)
        a = torch.sort(keys[valid]).values
        t = torch.maximum(a[min(K, n - 1)], keys.new_tensor(T))
        return t, valid & (keys < t)
    Kp = min(K, n)
    if Kp == 0:
        return keys.new_tensor(math.inf), torch.zeros_like(valid)
    v = torch.sort(keys[valid], descending=True).values[Kp - 1]
    return v, valid & (keys >= v)


def loss_of(view, lab_long, cw, align, keep, loss_weight, avg):
    """loss_weight / N * sum over keep of cw[l] nll; keep None: all valid pixels"""
    nll, _, wl, valid, _, _ = pieces(view, lab_long, cw, align)
    keep = valid if keep is None else keep.to(valid.device) & valid
    N = max(int(valid.sum()), 1) if avg else lab_long.numel()
    return torch.where(keep, wl * nll, torch.zeros_like(nll)).sum() * (loss_weight / N)


def held(name, got, yard, ref, figures):
    """error(got) <= 2 error(yard) + 2^-20 max |ref|; the figures are appended to `figures`"""
    e_got, e_yard = float((got - ref).abs().max()), float((yard - ref).abs().max())
    bound = 2.0 * e_yard + FLOOR * float(ref.abs().max())
    figures.append((name, e_got, e_yard, bound))
    return e_got <= bound


def report(tag, figures):
    worst = max(figures, key=lambda f: f[1] / f[3] if f[3] > 0 else 0.0)
    print("%s: %d figures, worst error/bound %.3f at %s (hip %.3e torch %.3e bound %.3e)"
          % (tag, len(figures), worst[1] / worst[3] if worst[3] > 0 else 0.0, worst[0], worst[1], worst[2], worst[3]))


def sampler_of(T, m):
    from mem_amd.seg_loss import OHEMPixelSampler
    return None if m is None else OHEMPixelSampler(T, m)


def hip(leaf, lab, layout, dims, align=False, cw=None, T=None, m=None, loss_weight=1.0, avg=False, mod=None):
    """the module on the GPU: loss, d loss / d leaf, counts, the stored keys, the threshold, the keep mask (all on the CPU)"""
    from mem_amd.seg_loss import SegCrossEntropy
    B, Cc, h, w = dims
    if mod is None:
        mod = SegCrossEntropy(IGN, align, loss_weight, avg, class_weight=cw, sampler=sampler_of(T, m))
    lh = leaf.detach().cuda().requires_grad_()
    labd = lab.cuda()
    loss = mod(make_view(lh, layout, B, Cc, h, w), labd)
    loss.backward()
    s = mod.last_stats
    counts = {k: int(s[k]) for k in ("n_valid", "n_correct", "n_bad", "n_kept")}
    keys = thr = keep = None
    if mod.sampler is not None:
        keys, thr = mod._keys(labd).cpu().clone(), s["threshold"].cpu().clone()
        keep = (keys >= 0) & ((keys < thr) if mod.sampler.thresh is not None else (keys >= thr))
    return dict(loss=loss.detach().cpu().double(), grad=lh.grad.cpu().double(), counts=counts, keys=keys, thr=thr, keep=keep, mod=mod)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach().cpu()


# ---------------------------------------------------------------- 1. the selection is exact
def key_patterns(gen, B, H, W):
    n = B * H * W
    shape = (B, H, W)
    u = torch.rand(shape, generator=gen)
    low = (torch.full(shape, 0.7).view(torch.int32) + torch.randint(0, 2, shape, generator=gen, dtype=torch.int32)).view(torch.float32)
    low4 = (torch.full(shape, 0.7).view(torch.int32) + torch.randint(0, 4, shape, generator=gen, dtype=torch.int32)).view(torch.float32)
    ends = u.clone()
    ends.view(-1)[0] = 0.0
    ends.view(-1)[n // 2] = 1.0
    ends.view(-1)[n - 1] = 0.0 if n > 2 else ends.view(-1)[n - 1]
    den = u.clone()
    den.view(-1)[n // 3] = 1e-40                                        # a denormal
    den.view(-1)[n - 1] = 2e-45
    half = u.clone()
    half[torch.rand(shape, generator=gen) < 0.5] = -1.0
    wide = torch.rand(shape, generator=gen) * torch.tensor([1e-3, 1.0, 30.0])[torch.randint(0, 3, shape, generator=gen)]   # nll-like
    return {"equal": torch.full(shape, 0.5), "lowbit": low, "lowbits": low4, "ends": ends, "denormal": den, "half_invalid": half,
            "none_valid": torch.full(shape, -1.0), "uniform": u, "wide": wide}


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (1, 1, 2), (1, 3, 85), (1, 16, 16), (1, 1, 257), (3, 36, 68)])
def test_selection_is_exact(B, H, W):
    from mem_amd import ops
    gen = torch.Generator().manual_seed(B * 1000 + H * W)
    ws = torch.empty(int(ops.seg_ohem_plan(B, 2, 1, 1, H, W, sampler=1, thresh=0.5, min_kept=1).ws_bytes), dtype=torch.uint8, device="cuda")
    ws.fill_(0xA5)                                                  # the call prepares its workspace itself
    thr, stats = torch.empty(1, device="cuda"), torch.full((4,), -7, dtype=torch.int64, device="cuda")
    checked, failures = 0, []
    for name, keys in key_patterns(gen, B, H, W).items():
        n = int((keys >= 0).sum())
        kd = keys.cuda()
        ms = sorted({0, 1, max(n - 1, 0) // B, n // B, (n + B - 1) // B, n // B + 1, n // (2 * B), 100000})
        a = torch.sort(keys[keys >= 0]).values
        for mode, m in itertools.product((1, 2), ms):
            K = m * B
            if mode == 1 and n > 0:
                kth = float(a[min(K, n - 1)])
                Ts = sorted({min(max(kth * 0.5, 1e-6), 1.0), min(max(kth, 1e-6), 1.0), min(kth * 1.5 + 0.01, 1.0), 1.0})    # below, at, above
            else:
                Ts = [0.7]
            for T in Ts:
                T32 = float(torch.tensor(T, dtype=torch.float32))
                want_t, want_keep = select(keys, mode, K, T32)
                ops.seg_ohem_select(kd, thr, stats, ws, mode, T if mode == 1 else None, m)
                got_t, got_n = thr.cpu(), int(stats[3])
                checked += 1
                if not (torch.equal(bits(got_t), bits(want_t.reshape(1))) and got_n == int(want_keep.sum())):
                    failures.append((name, mode, m, T, float(got_t), float(want_t), got_n, int(want_keep.sum())))
    print("selection %dx%dx%d: %d cases, %d failures" % (B, H, W, checked, len(failures)))
    assert not failures, failures[:10]
    assert tuple(int(v) for v in stats[:3]) == (-7, -7, -7)            # the selection writes stats[3] alone


# ---------------------------------------------------------------- 2. keys
@pytest.mark.parametrize("h,w,H,W", SHAPES)
def test_keys_within_twice_torchs_own_error(h, w, H, W):
    from mem_amd import ops
    figures, failures = [], []
    for Cc, layout, align, mode in itertools.product(CLASSES, ("nchw", "rows"), (False, True), (1, 2)):
        B = 2
        gen = torch.Generator().manual_seed(hash((h, w, H, W, Cc, align)) % (2 ** 31))
        leaf, lab, cw = make_leaf(gen, layout, B, Cc, h, w), make_labels(gen, B, Cc, H, W), make_weights(gen, Cc)
        ref, valid = keys_of(make_view(leaf.double(), layout, B, Cc, h, w), lab.long(), cw.double(), align, mode)
        yard, _ = keys_of(make_view(leaf.cuda(), layout, B, Cc, h, w), lab.cuda().long(), cw.cuda(), align, mode)
        keys, thr = torch.full((B, H, W), 7.0, device="cuda"), torch.zeros(1, device="cuda")
        ops.seg_ohem_keys(make_view(leaf.cuda(), layout, B, Cc, h, w), lab.cuda(), keys, thr, mode, cw.cuda() if mode == 2 else None,
                          IGN, align)
        got = keys.cpu()
        case = (Cc, layout, int(align), mode)
        ok = held(case, got.double(), yard.cpu().double(), ref, figures)
        ok &= bool((got[~valid] == -1.0).all()) and bool((got[valid] >= 0).all()) and float(thr) == 0.0
        if not ok:
            failures.append(case)
    report("keys %dx%d->%dx%d" % (h, w, H, W), figures)
    assert not failures, failures


# ---------------------------------------------------------------- 3. the keep mask against float64
@pytest.mark.parametrize("Cc", CLASSES)
@pytest.mark.parametrize("h,w,H,W", SHAPES)
def test_keep_mask_against_float64(h, w, H, W, Cc):
    failures, excused_max, cases = [], 0, 0
    for B, layout in ((1, "nchw"), (3, "rows"), (3, "nchw"), (1, "rows")):
        align = layout == "rows" and B == 3
        gen = torch.Generator().manual_seed(hash((h, w, H, W, Cc, B, layout == "rows")) % (2 ** 31))
        leaf, lab, cw = make_leaf(gen, layout, B, Cc, h, w), make_labels(gen, B, Cc, H, W), make_weights(gen, Cc)
        for T in (0.7, 0.3, None):
            mode = 2 if T is None else 1
            k64, _ = keys_of(make_view(leaf.double(), layout, B, Cc, h, w), lab.long(), cw.double(), align, mode)
            for m in (0, 5, 200, 100000):
                t64, keep64 = select(k64, mode, m * B, T if T is not None else 0.0)
                got = hip(leaf, lab, layout, (B, Cc, h, w), align, cw, T, m)
                differ = got["keep"] != keep64
                near = (k64 - t64).abs() <= 2.0 ** -16 * t64.abs() if math.isfinite(float(t64)) else torch.zeros_like(differ)
                n_diff, n_far = int(differ.sum()), int((differ & ~near).sum())
                cases += 1
                excused_max = max(excused_max, n_diff - n_far)
                ok = n_far == 0 and n_diff <= 2 and got["counts"]["n_kept"] == int(got["keep"].sum())
                if not ok:
                    failures.append((B, layout, T, m, n_diff, n_far, got["counts"]["n_kept"], int(got["keep"].sum()), int(keep64.sum())))
    print("keep mask %dx%d->%dx%d C=%d: %d cases, most excused pixels in one case %d" % (h, w, H, W, Cc, cases, excused_max))
    assert not failures, failures[:10]


# ---------------------------------------------------------------- 4. loss and gradient, on the HIP arm's own mask
MODES = [("weights", None, None), ("thresh", 0.7, 40), ("topk", None, 40)]


@pytest.mark.parametrize("h,w,H,W", SHAPES)
def test_loss_and_gradient_within_twice_torchs_own_error(h, w, H, W):
    from mem_amd.seg_loss import SegCrossEntropy
    figures, failures, dropped = [], [], set()
    for Cc, layout, avg, (name, T, m), weighted in itertools.product((2, 11, 19, 32), ("nchw", "rows"), (False, True), MODES, (True, False)):
        if name == "weights" and not weighted:
            continue
        B, align, lw = 3, Cc == 19, 0.4
        gen = torch.Generator().manual_seed(hash((h, w, H, W, Cc, layout == "rows")) % (2 ** 31))
        leaf, lab = make_leaf(gen, layout, B, Cc, h, w), make_labels(gen, B, Cc, H, W)
        cw = make_weights(gen, Cc) if weighted else None
        got = hip(leaf, lab, layout, (B, Cc, h, w), align, cw, T, m, lw, avg)
        keep = got["keep"]
        l64 = leaf.double().requires_grad_()
        ref = loss_of(make_view(l64, layout, B, Cc, h, w), lab.long(), None if cw is None else cw.double(), align, keep, lw, avg)
        ref.backward()
        l32 = leaf.cuda().requires_grad_()
        yard = loss_of(make_view(l32, layout, B, Cc, h, w), lab.cuda().long(), None if cw is None else cw.cuda(), align, keep, lw, avg)
        yard.backward()
        plain = hip(leaf, lab, layout, (B, Cc, h, w), align, None, None, None, lw, avg)["counts"]
        case = (Cc, layout, int(avg), name, int(weighted))
        ok = held(case + ("loss",), got["loss"], yard.detach().cpu().double(), ref.detach(), figures)
        ok &= held(case + ("dz",), got["grad"], l32.grad.cpu().double(), l64.grad, figures)
        ok &= bool(torch.isfinite(got["grad"]).all()) and all(got["counts"][k] == plain[k] for k in ("n_valid", "n_correct", "n_bad"))
        ok &= got["counts"]["n_kept"] == (int(keep.sum()) if keep is not None else plain["n_valid"])
        if m is not None:
            ok &= got["counts"]["n_kept"] > 0
            if got["counts"]["n_kept"] < plain["n_valid"]:
                dropped.add(name)
        if not ok:
            failures.append(case)
    report("loss %dx%d->%dx%d" % (h, w, H, W), figures)
    assert not failures, failures
    assert dropped == {"thresh", "topk"}                                          # both samplers did drop pixels somewhere


# ---------------------------------------------------------------- 5. bits
def _raw(fn, z, lab, **kw):
    """ops.seg_ce / ops.seg_ce_w on fresh outputs -> (dz, loss [3], stats)"""
    from mem_amd import ops
    B, Cc, h, w = z.shape
    n_stats = 3 if fn is ops.seg_ce else 4
    need = int(ops.seg_ohem_plan(B, Cc, h, w, lab.shape[1], lab.shape[2]).ws_bytes)
    dz, loss = torch.full_like(z, 9.0), torch.full((3,), 9.0, device="cuda")
    stats, ws = torch.full((n_stats,), -9, dtype=torch.int64, device="cuda"), torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    fn(z, lab, dz, loss, stats, ws, **kw)
    return dz, loss, stats


@pytest.mark.parametrize("Cc", [2, 11, 19, 32])
@pytest.mark.parametrize("avg", [False, True])
def test_nothing_on_and_all_ones_are_the_plain_loss_bit_for_bit(Cc, avg):
    from mem_amd import ops
    B, h, w, H, W = 3, 9, 17, 36, 68
    gen = torch.Generator().manual_seed(40 + Cc)
    z, lab = make_leaf(gen, "nchw", B, Cc, h, w).cuda(), make_labels(gen, B, Cc, H, W).cuda()
    want = _raw(ops.seg_ce, z, lab, avg_non_ignore=avg, loss_weight=0.4)
    for cw in (None, torch.ones(Cc, device="cuda")):
        got = _raw(ops.seg_ce_w, z, lab, avg_non_ignore=avg, loss_weight=0.4, class_weight=cw)
        assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[1]), bits(want[1]))
        assert torch.equal(got[2][:3], want[2]) and int(got[2][3]) == int(want[2][0])
    assert float(want[0].abs().max()) > 0 and not bool((want[0] == 9.0).any())


@pytest.mark.parametrize("T", [0.7, None])
def test_same_workspace_same_bits_across_calls_and_shapes(T):
    """two calls on one module (one workspace, one key buffer per shape), a smaller shape in between: a histogram left dirty,
    or a workspace region read before it is cleared, would change the second result"""
    from mem_amd.seg_loss import SegCrossEntropy
    gen = torch.Generator().manual_seed(50)
    big, small = (3, 11, 9, 17), (2, 11, 3, 5)
    leaf_b, lab_b, cw = make_leaf(gen, "nchw", *big), make_labels(gen, 3, 11, 36, 68), make_weights(gen, 11)
    leaf_s, lab_s = make_leaf(gen, "nchw", *small), make_labels(gen, 2, 11, 7, 11)
    mod = SegCrossEntropy(class_weight=cw, sampler=sampler_of(T, 40))
    runs = [hip(leaf_b, lab_b, "nchw", big, mod=mod), hip(leaf_b, lab_b, "nchw", big, mod=mod), hip(leaf_s, lab_s, "nchw", small, mod=mod),
            hip(leaf_b, lab_b, "nchw", big, mod=mod)]
    first = runs[0]
    assert 0 < first["counts"]["n_kept"] < first["counts"]["n_valid"]
    for r in (runs[1], runs[3]):
        assert torch.equal(r["loss"], first["loss"]) and torch.equal(r["grad"], first["grad"]) and r["counts"] == first["counts"]
        assert torch.equal(bits(r["thr"]), bits(first["thr"])) and torch.equal(bits(r["keys"]), bits(first["keys"]))
    fresh = hip(leaf_s, lab_s, "nchw", small, cw=cw, T=T, m=40)
    assert torch.equal(runs[2]["loss"], fresh["loss"]) and torch.equal(runs[2]["grad"], fresh["grad"]) and runs[2]["counts"] == fresh["counts"]


# ---------------------------------------------------------------- 6. edges
def _against_oracle(leaf, lab, dims, cw, T, m, avg=False):
    """the module against float64 and torch fp32 on the module's own mask -> (got, ok, figures)"""
    B, Cc, h, w = dims
    got = hip(leaf, lab, "nchw", dims, False, cw, T, m, 1.0, avg)
    l64 = leaf.double().requires_grad_()
    ref = loss_of(l64, lab.long(), None if cw is None else cw.double(), False, got["keep"], 1.0, avg)
    ref.backward()
    l32 = leaf.cuda().requires_grad_()
    yard = loss_of(l32, lab.cuda().long(), None if cw is None else cw.cuda(), False, got["keep"], 1.0, avg)
    yard.backward()
    figures = []
    ok = held("loss", got["loss"], yard.detach().cpu().double(), ref.detach(), figures) & held("dz", got["grad"], l32.grad.cpu().double(), l64.grad, figures)
    ok &= bool(torch.isfinite(got["loss"])) and bool(torch.isfinite(got["grad"]).all())
    # and the mask is float64's (these cases have no borderline pixel: the module's own, then the oracle's)
    k64, _ = keys_of(leaf.double(), lab.long(), None if cw is None else cw.double(), False, 2 if T is None else 1)
    t64, keep64 = select(k64, 2 if T is None else 1, m * B, T if T is not None else 0.0)
    return got, ok, figures, keep64


@pytest.mark.parametrize("T", [0.7, None])
@pytest.mark.parametrize("avg", [False, True])
def test_all_labels_ignored_with_a_sampler(T, avg):
    dims = (2, 11, 9, 17)
    gen = torch.Generator().manual_seed(60)
    leaf, cw = make_leaf(gen, "nchw", *dims), make_weights(gen, 11)
    lab = torch.full((2, 36, 68), IGN, dtype=torch.uint8)
    got = hip(leaf, lab, "nchw", dims, False, cw, T, 5, 1.0, avg)
    assert float(got["loss"]) == 0.0 and torch.equal(got["grad"], torch.zeros_like(got["grad"]))
    assert got["counts"] == dict(n_valid=0, n_correct=0, n_bad=0, n_kept=0)
    assert float(got["thr"]) == (-math.inf if T is not None else math.inf) and bool((got["keys"] == -1.0).all())
    assert float(got["mod"].acc_seg()) == 0.0


@pytest.mark.parametrize("T", [0.7, None])
def test_one_valid_pixel(T):
    dims = (2, 11, 9, 17)
    gen = torch.Generator().manual_seed(61)
    leaf, cw = make_leaf(gen, "nchw", *dims), torch.full((11,), 1.5)
    lab = torch.full((2, 36, 68), IGN, dtype=torch.uint8)
    lab[1, 35, 67] = 4
    for m in (0, 1, 5):
        got, ok, figures, keep64 = _against_oracle(leaf, lab, dims, cw, T, m)
        print("one pixel", T, m, figures, got["counts"])
        assert ok and torch.equal(got["keep"], keep64) and got["counts"]["n_valid"] == 1
        # thresh: n - 1 = 0 is the rank whatever m is, t = max(p, T), the pixel is kept when p < T; top-k: kept when K >= 1
        p = float(got["keys"][1, 35, 67])
        assert got["counts"]["n_kept"] == (int(p < 0.7) if T is not None else int(m >= 1))


def test_min_kept_zero_keeps_nothing_in_topk_and_k_beyond_n_keeps_all():
    dims = (3, 11, 9, 17)
    gen = torch.Generator().manual_seed(62)
    leaf, lab, cw = make_leaf(gen, "nchw", *dims), make_labels(gen, 3, 11, 36, 68), make_weights(gen, 11)
    none = hip(leaf, lab, "nchw", dims, False, cw, None, 0)
    assert float(none["loss"]) == 0.0 and not bool(none["grad"].any()) and none["counts"]["n_kept"] == 0 and float(none["thr"]) == math.inf
    assert none["counts"]["n_valid"] > 0
    weighted = hip(leaf, lab, "nchw", dims, False, cw, None, None)
    n = weighted["counts"]["n_valid"]
    for m in ((n + 2) // 3, n, 100000):                               # K = 3 m >= n
        allk = hip(leaf, lab, "nchw", dims, False, cw, None, m)
        assert allk["counts"]["n_kept"] == n and allk["counts"] == weighted["counts"]
        assert torch.equal(allk["loss"], weighted["loss"]) and torch.equal(allk["grad"], weighted["grad"])       # bit for bit
    got, ok, figures, keep64 = _against_oracle(leaf, lab, dims, cw, None, 100000)
    assert ok and torch.equal(got["keep"], keep64), figures
    # thresh with K >= n: t = max(the largest key, T); everything below it
    got, ok, figures, keep64 = _against_oracle(leaf, lab, dims, cw, 0.7, 100000)
    assert ok and torch.equal(got["keep"], keep64) and got["counts"]["n_kept"] >= n - 2, figures


@pytest.mark.parametrize("T", [0.7, None])
def test_a_logit_of_1e4_stays_finite_and_matches(T):
    dims = (1, 11, 9, 17)
    gen = torch.Generator().manual_seed(63)
    leaf, lab, cw = make_leaf(gen, "nchw", *dims), make_labels(gen, 1, 11, 36, 68), make_weights(gen, 11)
    leaf[0, 3, 4, 8] = 1e4
    cw[3] = 2.0
    got, ok, figures, keep64 = _against_oracle(leaf, lab, dims, cw, T, 40)
    print("1e4", T, figures, got["counts"])
    assert ok and bool(torch.isfinite(got["keys"]).all()) and math.isfinite(float(got["thr"]))
    # the mask is float64's, but for at most 2 pixels whose float64 key lies within a relative 2^-16 of the float64 threshold
    mode = 2 if T is None else 1
    k64, _ = keys_of(leaf.double(), lab.long(), cw.double(), False, mode)
    t64, _ = select(k64, mode, 40 * dims[0], T if T is not None else 0.0)
    differ = got["keep"] != keep64
    near = (k64 - t64).abs() <= 2.0 ** -16 * t64.abs()
    assert int((differ & ~near).sum()) == 0 and int(differ.sum()) <= 2
    assert 0 < got["counts"]["n_kept"] < got["counts"]["n_valid"]


# ---------------------------------------------------------------- 7. bounds
@pytest.mark.parametrize("h,w,H,W", [(3, 5, 7, 11), (9, 17, 36, 68), (17, 9, 68, 36)])
@pytest.mark.parametrize("mode", [1, 2])
def test_nothing_is_written_outside_the_outputs_and_the_workspace(h, w, H, W, mode):
    from mem_amd import ops
    B, Cc, pad = 3, 11, 256
    gen = torch.Generator().manual_seed(70)
    z, lab, cw = make_leaf(gen, "nchw", B, Cc, h, w).cuda(), make_labels(gen, B, Cc, H, W).cuda(), make_weights(gen, Cc).cuda()
    T = 0.7 if mode == 1 else None
    need = int(ops.seg_ohem_plan(B, Cc, h, w, H, W, sampler=mode, thresh=T, min_kept=40).ws_bytes)
    sizes = dict(dz=z.numel(), keys=B * H * W, thr=1, loss=3)
    big = {k: torch.full((pad + n + pad,), 777.0, device="cuda") for k, n in sizes.items()}
    big_ws = torch.full((pad + need + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    big_stats = torch.full((pad + 4 + pad,), -777, dtype=torch.int64, device="cuda")
    inner = {k: big[k][pad:pad + n] for k, n in sizes.items()}
    dz, keys, ws, stats = inner["dz"].view(B, Cc, h, w), inner["keys"].view(B, H, W), big_ws[pad:pad + need], big_stats[pad:pad + 4]
    ops.seg_ohem_keys(z, lab, keys, inner["thr"], mode, cw, IGN, False)
    ops.seg_ohem_select(keys, inner["thr"], stats, ws, mode, T, 40, (Cc, h, w))
    n_sel = int(stats[3])
    ops.seg_ce_w(z, lab, dz, inner["loss"], stats, ws, class_weight=cw, sampler=mode, keys=keys, threshold=inner["thr"])
    torch.cuda.synchronize()
    for k, n in sizes.items():
        assert bool((big[k][:pad] == 777.0).all()) and bool((big[k][pad + n:] == 777.0).all()), k
        assert not bool((inner[k] == 777.0).any()), k                   # and what is inside was written
    assert bool((big_ws[:pad] == 0xA5).all()) and bool((big_ws[pad + need:] == 0xA5).all())
    assert bool((big_stats[:pad] == -777).all()) and bool((big_stats[pad + 4:] == -777).all())
    # the three calls agree: the selection's n_kept is the loss kernel's, and the definition's on the stored keys
    k_cpu = keys.cpu()
    want_t, want_keep = select(k_cpu, mode, 40 * B, T if T is not None else 0.0)
    assert torch.equal(bits(inner["thr"]), bits(want_t.reshape(1)))
    assert n_sel == int(stats[3]) == int(want_keep.sum()) and 0 < n_sel <= int(stats[0])
    ref = loss_of(z.cpu().double(), lab.cpu().long(), cw.cpu().double(), False, want_keep, 1.0, False)
    assert float(inner["loss"][0]) == pytest.approx(float(ref), rel=1e-5)


# ---------------------------------------------------------------- 8. through a head
def test_through_a_head_both_arms():
    from mem_amd import ops
    from mem_amd.seg_heads import FCNHead
    B, Cin, C, K, h, w, H, W, p = 2, 64, 64, 5, 8, 8, 32, 32, 0.1
    KEY = (20240229, 7)
    gen = torch.Generator().manual_seed(80)
    x = (torch.randn(B, Cin, h, w, generator=gen) * 1.5).to(torch.bfloat16).float()
    sd = {"convs.0.conv.weight": (torch.randn(C, Cin, 3, 3, generator=gen) * (2.0 / (9 * Cin)) ** 0.5).to(torch.bfloat16).float(),
          "convs.0.bn.weight": 1.0 + 0.3 * torch.randn(C, generator=gen), "convs.0.bn.bias": 0.3 * torch.randn(C, generator=gen),
          "convs.0.bn.running_mean": 0.2 * torch.randn(C, generator=gen), "convs.0.bn.running_var": 0.5 + torch.rand(C, generator=gen),
          "convs.0.bn.num_batches_tracked": torch.tensor(3),
          "conv_seg.weight": torch.randn(K, C, 1, 1, generator=gen) * 3.0 * (1.0 / C) ** 0.5, "conv_seg.bias": 0.1 * torch.randn(K, generator=gen)}
    lab = torch.randint(0, K, (B, H, W), generator=gen)
    lab[torch.rand((B, H, W), generator=gen) < 0.2] = IGN
    cfg = dict(type="CrossEntropyLoss", loss_weight=0.4, class_weight=[1.0, 2.5, 0.0, 0.5, 1.5],
               sampler=dict(type="OHEMPixelSampler", thresh=0.7, min_kept=50))
    keep = torch.empty((B, C), dtype=torch.uint8, device="cuda")
    ops.dropout_mask(ops.dropout_params(KEY[0], KEY[1], ops.DROPOUT_SITE_HEAD, p), 0, B, C, keep)
    names = ["convs.0.conv.weight", "convs.0.bn.weight", "convs.0.bn.bias", "conv_seg.weight", "conv_seg.bias"]

    def run(impl, device, dtype, autocast=False, loss_decode=cfg):
        kw = dict(loss_decode=loss_decode) if loss_decode is not None else dict(loss_weight=0.4)
        head = FCNHead(in_channels=Cin, channels=C, num_classes=K, in_index=0, dropout_ratio=p, impl=impl, **kw)
        head.load_state_dict(sd, strict=True)
        head = head.to(device=device, dtype=dtype).train()
        head.drop_key, head.keep_mask = KEY, keep.to(device)
        xg = x.to(device=device, dtype=dtype).requires_grad_()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            out = head.forward_train((xg,), lab.to(device))
        out["loss_seg"].float().backward()
        params = dict(head.named_parameters())
        grads = [xg.grad] + [params[n].grad for n in names]
        return (out["loss_seg"].detach().double().cpu(), [g.detach().double().cpu() for g in grads], float(out["acc_seg"]),
                int(head.loss_decode.last_stats["n_kept"]), int(head.loss_decode.last_stats["n_valid"]))

    ref = run("torch", "cpu", torch.float64)
    yard = run("torch", "cuda", torch.float32, autocast=True)
    got = run("hip", "cuda", torch.float32)
    figures = []
    ok = [held("loss_seg", got[0], yard[0], ref[0], figures)]
    ok += [held("d " + n, a, b, c, figures) for n, a, b, c in zip(["map"] + names, got[1], yard[1], ref[1])]
    for f in figures:
        print("head %-22s hip %.3e  torch bf16 %.3e  bound %.3e" % f)
    print("n_kept: float64 %d, bf16 autocast %d, hip %d of %d valid" % (ref[3], yard[3], got[3], got[4]))
    assert all(ok), [f for f, o in zip(figures, ok) if not o]
    assert 0 < got[3] < got[4] and ref[4] == got[4]
    # acc_seg is taken over all valid pixels: the head with the plain loss reports the same
    plain = run("hip", "cuda", torch.float32, loss_decode=None)
    assert plain[2] == got[2] and plain[4] == got[4] and plain[3] == plain[4]
    assert float(plain[0]) != float(got[0])
