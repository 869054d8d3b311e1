"""-m gpu: the PSP decode head on the device.  The five pyramid-pooling kernels each against float64 on the kernel's own stored
inputs, under bounds read off the code: an fp32 output is held to (its longest chain of fp32 roundings) x 2^-24 x (the sum of the
magnitudes of its terms), a bf16 output to 2^-8 relative in addition; a ReLU gate whose float64 pre-activation lies within fp32
rounding of zero may fall either way and its whole term joins the bounds it enters (tests/test_psp_head_cpu.py counts them).
Then PSPHead(impl="hip") forward and every gradient against the float64 torch arm fed the same bf16-valued map, the same
weights and the same Dropout2d mask, under the project's yardstick:

    error(hip) <= 2 x error(torch arm under bf16 autocast on the GPU, same inputs) + 2^-20 x max |float64 result|

Measured ratios per case: DESIGN.md section 2c, "PSP decode head"."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_psp_head_cpu import CASES, U, bn_terms, kernel_inputs, param_names, pool_matrix, state, tables_of
from test_seg_head_gpu import FLOOR, GUARD, KEY, _guarded, _guards_intact, _labels, _mask, held, report

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
KERNEL_CASES = ["P1", "P2", "P3", "P4", "P5", "BIG"]
HEAD_CASES = ["P1", "P2", "P3", "P4", "P5"]


# ---------------------------------------------------------------------------------------------- padded buffers
def _padded_in(vals):
    """vals bf16 [B, m, m', ch] on the CPU -> the padded format on the device with a NaN ring (a ring that must not be read)"""
    B, m, mm, ch = vals.shape
    buf = torch.full((B, m + 2, mm + 2, ch), float("nan"), dtype=torch.bfloat16, device="cuda")
    buf[:, 1:-1, 1:-1] = vals.cuda()
    return buf


def _padded_out(B, m, mm, ch):
    """(guarded flat buffer, its padded view), every element the sentinel: the ring must keep it, the guards stay NaN"""
    big, flat = _guarded(B * (m + 2) * (mm + 2) * ch, torch.bfloat16)
    flat.fill_(SENTINEL)
    return big, flat.view(B, m + 2, mm + 2, ch)


def _ring_kept(buf):
    ring = torch.ones(buf.shape[:3], dtype=torch.bool, device=buf.device)
    ring[:, 1:-1, 1:-1] = False
    return bool((buf[ring] == SENTINEL).all())


def _worst(name, err, bound):
    worst = float((err / (bound + 1e-30)).max())
    print("    %-10s worst error / bound %.4f (largest error %.3e)" % (name, worst, float(err.max())))
    return worst


def _vectors(inp):
    return [inp[k].cuda() for k in ("mean", "rstd", "gamma", "beta")]


# ---------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("case", KERNEL_CASES)
def test_pool_against_float64(case):
    """a bin of n pixels: n additions (the first one, to -0, exact), the division, then bf16: (n + 1) 2^-24 x mean |x| + 2^-8 |mean|"""
    from mem_amd import ops
    B, Cin, C, K, h, w, scales = CASES[case]
    inp = kernel_inputs(case)
    x = inp["x"].cuda()
    outs = [_padded_out(B, s, s, Cin) for s in scales]
    ops.ppm_pool(x, scales, [o[1] for o in outs])
    first = [o[1].clone() for o in outs]
    x64 = inp["x"].double()
    print(case, "pool")
    for s, (big, P) in zip(scales, outs):
        Ay, Ax = pool_matrix(h, s), pool_matrix(w, s)
        want = torch.einsum("iy,bcyx,jx->bijc", Ay, x64, Ax)
        mag = torch.einsum("iy,bcyx,jx->bijc", Ay, x64.abs(), Ax)
        cnt = ((Ay > 0).sum(1)[:, None] * (Ax > 0).sum(1)[None, :]).double()[None, :, :, None]
        err = (P[:, 1:-1, 1:-1].double().cpu() - want).abs()
        assert _worst("scale %d" % s, err, (cnt + 1) * U * mag + 2.0 ** -8 * want.abs()) <= 1.0
        assert _ring_kept(P) and _guards_intact(big)
        if s == h == w:                                                   # a bin is a pixel: the mover's bits
            same = ops.map_to_nhwc_pad(x, torch.zeros_like(P))
            assert torch.equal(P[:, 1:-1, 1:-1].view(torch.int16), same[:, 1:-1, 1:-1].view(torch.int16))
    if case == "P5":
        assert scales == (h,) == (w,)
    ops.ppm_pool(x, scales, [o[1] for o in outs])
    assert all(torch.equal(a.view(torch.int16), o[1].view(torch.int16)) for a, o in zip(first, outs))      # two calls, the same bits


@pytest.mark.parametrize("case", KERNEL_CASES)
def test_concat_fwd_against_float64(case):
    """channel Cin + i C + c: xhat (2 roundings), u (1), the weights 1 - w1 (1 each), five products and sums: 12 covers the
    chain; the terms are those of u at the four taps, under the bilinear weights.  The forward is continuous in u: a gate at
    zero adds nothing.  The map's channels are the mover's bits."""
    from mem_amd import ops
    B, Cin, C, K, h, w, scales = CASES[case]
    n = len(scales)
    inp = kernel_inputs(case)
    x = inp["x"].cuda()
    Y = [_padded_in(y) for y in inp["Y"]]
    big, xcat = _padded_out(B, h, w, Cin + n * C)
    ops.ppm_concat_fwd(x, scales, Y, *_vectors(inp), xcat)
    first = xcat.clone()
    assert _ring_kept(xcat) and _guards_intact(big)
    same = ops.map_to_nhwc_pad(x, torch.zeros((B, h + 2, w + 2, Cin), dtype=torch.bfloat16, device="cuda"))
    assert torch.equal(xcat[:, 1:-1, 1:-1, :Cin].contiguous().view(torch.int16), same[:, 1:-1, 1:-1].contiguous().view(torch.int16))
    print(case, "concat_fwd")
    got = xcat[:, 1:-1, 1:-1].double().cpu()
    for i, (s, (My, Mx, _, _)) in enumerate(zip(scales, tables_of(case))):
        xh, u, mag_xh, mag_u, amb = bn_terms(inp, i)
        want = torch.einsum("yi,bijc,xj->byxc", My, u.clamp(min=0.0), Mx)
        mag = torch.einsum("yi,bijc,xj->byxc", My, mag_u, Mx)
        err = (got[..., Cin + i * C:Cin + (i + 1) * C] - want).abs()
        assert _worst("scale %d" % s, err, 12 * U * mag + 2.0 ** -8 * want.abs()) <= 1.0
        if s == h:
            assert bool((My == torch.eye(h, dtype=torch.float64)).all())  # an identity axis: every w1 is 0
    xcat.fill_(SENTINEL)
    ops.ppm_concat_fwd(x, scales, Y, *_vectors(inp), xcat)
    assert torch.equal(first.view(torch.int16), xcat.view(torch.int16))


@pytest.mark.parametrize("case", KERNEL_CASES)
def test_concat_bwd_sums_against_float64(case):
    """dA of a bin: N = (hi - lo + 1) of both axes terms, each the product of two weights (1 - w1 and the sum of a clamped pair:
    2 roundings) and one fused multiply-add: N + 4.  A channel sum: a row lane's chain ceil(rows / 32), the 32 lanes, the
    roundings of g behind it, and 4 for xhat and its product."""
    from mem_amd import ops
    B, Cin, C, K, h, w, scales = CASES[case]
    n = len(scales)
    inp = kernel_inputs(case)
    dxcat = _padded_in(inp["dxcat"])
    Y = [_padded_in(y) for y in inp["Y"]]
    gb = [_guarded(B * s * s * C, torch.float32) for s in scales]
    g = [flat.view(B * s * s, C) for (_, flat), s in zip(gb, scales)]
    bigs, sflat = _guarded(n * 2 * C, torch.float32)
    sums = sflat.view(n, 2, C)
    ops.ppm_concat_bwd_sums(dxcat, Cin, scales, Y, *_vectors(inp), g, sums)
    first = [t.clone() for t in g] + [sums.clone()]
    assert _guards_intact(bigs) and all(_guards_intact(b) for b, _ in gb)
    d64 = inp["dxcat"].double()
    print(case, "concat_bwd_sums")
    n_amb = n_all = 0
    for i, (s, (My, Mx, ty, tx)) in enumerate(zip(scales, tables_of(case))):
        xh, u, mag_xh, mag_u, amb = bn_terms(inp, i)
        d = d64[..., Cin + i * C:Cin + (i + 1) * C]
        dA = torch.einsum("yi,byxc,xj->bijc", My, d, Mx)
        mag = torch.einsum("yi,byxc,xj->bijc", My, d.abs(), Mx)
        ny, nx = torch.tensor(ty[3] - ty[2] + 1), torch.tensor(tx[3] - tx[2] + 1)
        Lg = ((ny[:, None] * nx[None, :]).double() + 4)[None, :, :, None]
        slack = amb * dA.abs()
        want_g = dA * (u > 0)
        err = (g[i].double().cpu().view(B, s, s, C) - want_g).abs()
        assert _worst("g, scale %d" % s, err, Lg * U * mag + slack) <= 1.0
        L = float(Lg.max()) + -(-B * s * s // 32) + 32
        want = torch.stack([want_g.sum((0, 1, 2)), (want_g * xh).sum((0, 1, 2))])
        bound = torch.stack([L * U * mag.sum((0, 1, 2)) + slack.sum((0, 1, 2)),
                             (L + 4) * U * (mag * mag_xh).sum((0, 1, 2)) + (slack * mag_xh).sum((0, 1, 2))])
        assert _worst("sums, scale %d" % s, (sums[i].double().cpu() - want).abs(), bound) <= 1.0
        n_amb, n_all = n_amb + int(amb.sum()), n_all + amb.numel()
    print("    %d of %d gates within fp32 rounding of zero" % (n_amb, n_all))
    assert n_amb <= 1e-3 * n_all
    for t in g + [sums]:
        t.fill_(float("nan"))
    ops.ppm_concat_bwd_sums(dxcat, Cin, scales, Y, *_vectors(inp), g, sums)
    assert all(torch.equal(a, b) for a, b in zip(first, g + [sums]))


@pytest.mark.parametrize("case", KERNEL_CASES)
def test_bwd_apply_against_float64(case):
    """gamma rstd (g - tot0 inv_n - xhat tot1 inv_n): ten roundings at most behind the bf16 one; tot None: no correction terms"""
    from mem_amd import ops
    B, Cin, C, K, h, w, scales = CASES[case]
    inp = kernel_inputs(case)
    Y = [_padded_in(y) for y in inp["Y"]]
    g = [t.cuda() for t in inp["g"]]
    print(case, "bwd_apply")
    for tot in (inp["tot"], None):
        outs = [_padded_out(B, s, s, C) for s in scales]
        ops.ppm_bwd_apply(g, scales, Y, *_vectors(inp), None if tot is None else tot.cuda(), inp["inv_n"], [o[1] for o in outs], (h, w))
        for i, (s, (big, dY)) in enumerate(zip(scales, outs)):
            xh, u, mag_xh, mag_u, amb = bn_terms(inp, i)
            gi = inp["g"][i].double().view(B, s, s, C)
            t0, t1 = (0.0, 0.0) if tot is None else (tot[i, 0].double() * inp["inv_n"][i], tot[i, 1].double() * inp["inv_n"][i])
            sc = inp["gamma"][i].double() * inp["rstd"][i].double()
            want = sc * (gi - t0 - xh * t1)
            t0a, t1a = (0.0, 0.0) if tot is None else (t0.abs(), t1.abs())
            bound = 2.0 ** -8 * want.abs() + 10 * U * sc.abs() * (gi.abs() + t0a + mag_xh * t1a)
            err = (dY[:, 1:-1, 1:-1].double().cpu() - want).abs()
            assert _worst("scale %d%s" % (s, "" if tot is not None else " eval"), err, bound) <= 1.0
            assert _ring_kept(dY) and _guards_intact(big)
    again = [_padded_out(B, s, s, C) for s in scales]
    ops.ppm_bwd_apply(g, scales, Y, *_vectors(inp), None, inp["inv_n"], [o[1] for o in again], (h, w))
    assert all(torch.equal(a[1].view(torch.int16), b[1].view(torch.int16)) for a, b in zip(outs, again))


@pytest.mark.parametrize("case", KERNEL_CASES)
def test_dmap_against_float64(case):
    """f32(dXcat) plus at most 2 x 2 bins per scale, each a division and an addition: 8 n + 1 roundings"""
    from mem_amd import ops
    B, Cin, C, K, h, w, scales = CASES[case]
    n = len(scales)
    inp = kernel_inputs(case)
    dxcat = _padded_in(inp["dxcat"])
    dP = [_padded_in(p) for p in inp["dP"]]
    big, flat = _guarded(B * Cin * h * w, torch.float32)
    out = ops.ppm_dmap(dxcat, Cin, scales, dP, flat.view(B, Cin, h, w))
    first = out.clone()
    want = inp["dxcat"].double()[..., :Cin].permute(0, 3, 1, 2).clone()
    mag = want.abs()
    most = 0
    for s, p in zip(scales, inp["dP"]):
        Ay, Ax = pool_matrix(h, s), pool_matrix(w, s)
        want += torch.einsum("iy,bijc,jx->bcyx", Ay, p.double(), Ax)
        mag += torch.einsum("iy,bijc,jx->bcyx", Ay, p.double().abs(), Ax)
        most = max(most, int((Ay > 0).sum(0).max()) * int((Ax > 0).sum(0).max()))
    print(case, "dmap (at most %d bins of a scale hold a pixel)" % most)
    assert most <= 4 and _guards_intact(big)
    assert _worst("dmap", (out.double().cpu() - want).abs(), (8 * n + 1) * U * mag) <= 1.0
    if scales == (h,) == (w,):                                            # P5: every bin is one pixel, the sum of two bf16 values
        assert torch.equal(out.cpu(), (inp["dxcat"][..., :Cin].float() + inp["dP"][0].float()).permute(0, 3, 1, 2))
    flat.fill_(float("nan"))
    assert torch.equal(ops.ppm_dmap(dxcat, Cin, scales, dP, flat.view(B, Cin, h, w)), first)


# ---------------------------------------------------------------------------------------------- the head against float64
def _names(case):
    return ["x"] + param_names(len(CASES[case][6]))


def _head(case, impl, sd, p, train=True, device="cuda", dtype=None):
    from mem_amd.seg_heads import PSPHead
    B, Cin, C, K, h, w, scales = CASES[case]
    head = PSPHead(in_channels=Cin, channels=C, num_classes=K, in_index=0, pool_scales=scales, dropout_ratio=p, impl=impl)
    head.load_state_dict(sd, strict=True)
    head.drop_key = KEY
    if dtype is not None:
        head = head.to(dtype)
    return head.to(device).train(train)


def _run(head, x, gout, autocast=False, names=None):
    """logits and the gradients of one forward + backward, on the head's device"""
    dev = head.conv_seg.weight.device
    head.zero_grad(set_to_none=True)
    xg = x.to(dev, head.conv_seg.weight.dtype).requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        out = head((xg,))
    if out.dtype == torch.float64:
        out.backward(gout.to(dev, torch.float64))
    else:
        out.float().backward(gout.to(dev))
    ps = dict(head.named_parameters())
    grads = [xg.grad] + [ps[n].grad for n in names[1:]]
    return out.detach().clone(), [g.detach().clone() for g in grads]


@functools.lru_cache(maxsize=None)
def _reference(case, p, train=True):
    """the torch arm in float64 on the CPU, once per case: logits and gradients, with the mask of the contract"""
    B, Cin, C, K, h, w, scales = CASES[case]
    x, sd, gout = state(case)
    keep = _mask(B, C, p).cpu() if (train and p > 0.0) else None
    ref = _head(case, "torch", sd, p, train, device="cpu", dtype=torch.float64)
    ref.keep_mask = keep
    out, grads = _run(ref, x, gout, names=_names(case))
    return out, grads, keep


def _against_reference(case, p, train=True):
    x, sd, gout = state(case)
    names = _names(case)
    ref_out, ref_grads, keep = _reference(case, p, train)
    hip_out, hip_grads = _run(_head(case, "hip", sd, p, train), x, gout, names=names)
    yard = _head(case, "torch", sd, p, train)
    yard.keep_mask = None if keep is None else keep.cuda()
    yard_out, yard_grads = _run(yard, x, gout, autocast=True, names=names)
    figures = []
    ok = [held("logits", hip_out, yard_out, ref_out, figures)]
    ok += [held("d " + n, a, b, c, figures) for n, a, b, c in zip(names, hip_grads, yard_grads, ref_grads)]
    report("%s p=%.1f %s" % (case, p, "train" if train else "eval"), figures)
    return ok, figures, (hip_out, ref_out, keep)


@pytest.mark.parametrize("case", HEAD_CASES)
def test_forward_and_backward_within_twice_torchs_own_error(case):
    ok, figures, _ = _against_reference(case, 0.1)
    assert all(ok), [f for f, o in zip(figures, ok) if not o]


def test_dropout2d_follows_the_mask_contract():
    """p = 0.5: the logits agree with the reference fed memhip_dropout_mask(d, 0, B, C)'s bits; one wrong bit moves its sample
    beyond the comparison's bound and no other sample"""
    case = "P2"
    B, Cin, C, K, h, w, scales = CASES[case]
    ok, figures, (hip_out, ref_out, keep) = _against_reference(case, 0.5)
    kept = float(keep.float().mean())
    print("keep rate %.3f over %d (sample, channel) pairs" % (kept, B * C))
    assert all(ok), [f for f, o in zip(figures, ok) if not o]
    assert 0.35 < kept < 0.65 and not bool((keep[0] == keep[1]).all())
    x, sd, gout = state(case)
    wrong = keep.clone()
    wrong[1, 5] ^= 1
    off_head = _head(case, "torch", sd, 0.5, device="cpu", dtype=torch.float64)
    off_head.keep_mask = wrong
    with torch.no_grad():
        off = off_head((x.double(),))
    bound = figures[0][3]
    moved = (off - ref_out).abs().amax(dim=(1, 2, 3))
    print("one flipped bit moves sample 1 by %.3e (bound of the comparison %.3e), the others by %.3e" % (float(moved[1]), bound, float(moved[[0, 2, 3]].max())))
    assert float(moved[1]) > 4 * bound and float(moved[[0, 2, 3]].max()) == 0.0


def test_two_calls_give_the_same_bits():
    case = "P2"
    x, sd, gout = state(case)
    head = _head(case, "hip", sd, 0.1)
    a_out, a_grads = _run(head, x, gout, names=_names(case))
    b_out, b_grads = _run(head, x, gout, names=_names(case))
    assert torch.equal(a_out, b_out) and all(torch.equal(a, b) for a, b in zip(a_grads, b_grads))
    assert all(bool(torch.isfinite(g).all()) for g in a_grads)


def test_eval_mode_uses_the_five_running_statistics_and_changes_none():
    case = "P1"
    x, sd, gout = state(case)
    ok, figures, _ = _against_reference(case, 0.1, train=False)
    assert all(ok), [f for f, o in zip(figures, ok) if not o]
    head = _head(case, "hip", sd, 0.1, train=False)
    with torch.no_grad():
        out = head((x.cuda(),))
    ref_out = _reference(case, 0.1, False)[0]
    print("eval, no_grad: max error %.3e" % float((out.double().cpu() - ref_out).abs().max()))
    assert not out.requires_grad and float((out.double().cpu() - ref_out).abs().max()) <= 2.0 ** -7 * float(ref_out.abs().max())
    now = head.state_dict()
    stats = [k for k in sd if "running_" in k or "num_batches" in k]
    assert len(stats) == 15 and all(torch.equal(now[k].cpu(), sd[k]) for k in stats)
    used = sorted(k[0] for k in head._bufs)
    print("buffers of an eval forward under no_grad:", used)
    n = len(CASES[case][6])
    assert used == sorted(["logits", "xcat", "y"] + ["ppm.p%d" % i for i in range(n)] + ["ppm.y%d" % i for i in range(n)])
    head.train()
    head((x.cuda().requires_grad_(),))
    now = head.state_dict()
    assert all(int(now[k]) == 4 for k in stats if "num_batches" in k)
    assert not any(torch.equal(now[k].cpu(), sd[k]) for k in stats if "running_" in k)


def test_running_statistics_match_batchnorm():
    """two training forwards: the five batch norms' running statistics of the hip arm against torch's batch norm in float64
    (the torch arm, on the same maps): fp32 statistics of bf16-rounded values, 2^-9 relative on every value at most, so 2^-8 of
    the spread is ample"""
    case = "P2"
    x, sd, gout = state(case)
    head = _head(case, "hip", sd, 0.1)
    ref = _head(case, "torch", sd, 0.0, device="cpu", dtype=torch.float64)
    for i in range(2):
        xi = (x * (1.0 + i)).to(torch.bfloat16).float()
        with torch.no_grad():
            head((xi.cuda(),))
            ref((xi.double(),))
    got, want = head.state_dict(), ref.state_dict()
    for pre in ["psp_modules.%d.1.bn." % i for i in range(4)] + ["bottleneck.bn."]:
        em = float((got[pre + "running_mean"].double().cpu() - want[pre + "running_mean"]).abs().max())
        ev = float((got[pre + "running_var"].double().cpu() - want[pre + "running_var"]).abs().max())
        print("%-22s running mean error %.3e, running var error %.3e" % (pre, em, ev))
        assert int(got[pre + "num_batches_tracked"]) == 5 == int(want[pre + "num_batches_tracked"])
        assert em <= 2.0 ** -8 * float(want[pre + "running_var"].sqrt().max()) and ev <= 2.0 ** -8 * float(want[pre + "running_var"].max())


def test_a_second_step_sees_the_optimizers_weights():
    """the bf16 weight copies follow torch's version counter: after optimizer.step() the next forward is that of a fresh head
    holding the new state dict, bit for bit, and not the first step's"""
    case = "P1"
    x, sd, gout = state(case)
    names = _names(case)
    head = _head(case, "hip", sd, 0.1)
    opt = torch.optim.SGD(head.parameters(), lr=0.01)
    out1, _ = _run(head, x, gout, names=names)
    opt.step()
    out2, grads2 = _run(head, x, gout, names=names)
    fresh = _head(case, "hip", {k: v.detach().cpu().clone() for k, v in head.state_dict().items()}, 0.1)
    out3, grads3 = _run(fresh, x, gout, names=names)
    moved = float((out2 - out1).abs().max())
    print("the step moved the logits by %.3e" % moved)
    assert moved > 1e-3 and torch.equal(out2, out3) and all(torch.equal(a, b) for a, b in zip(grads2, grads3))


# ---------------------------------------------------------------------------------------------- SyncBN hook
def test_syncbn_hook_two_identical_ranks():
    """reduce doubles the sums (two ranks holding the same batch): the result is the single-rank run on the batch
    concatenated with itself.  FCNHead's test and its two tolerances: the statistics of the two runs are added in different
    orders (relative differences of a few 2^-24 on mean and rstd), so fp32 results -- the logits, the gradients of the
    bottleneck's batch norm and of conv_seg, every running statistic -- agree to 1e-5 of their largest value; what passes a bf16
    gradient (dY of the bottleneck, then dXcat and dY_s: the map, every convolution weight and the pyramid's batch norms), where
    such a difference can move single elements by one bf16 step (2^-8 relative), agrees to 2^-7."""
    case = "P2"
    B, Cin, C, K, h, w, scales = CASES[case]
    x, sd, gout = state(case)
    names = _names(case)
    calls = []

    def doubled(vec, tag):
        calls.append(tag)
        return vec * 2.0

    rank = _head(case, "hip", sd, 0.0)
    rank.reduce = doubled
    r_out, r_grads = _run(rank, x, gout, names=names)
    full = _head(case, "hip", sd, 0.0)
    f_out, f_grads = _run(full, torch.cat([x, x]), torch.cat([gout, gout]), names=names)
    assert calls == ["stats", "stats", "bwd", "bwd"]
    fp32 = {"bottleneck.bn.weight", "bottleneck.bn.bias", "conv_seg.weight", "conv_seg.bias"}
    e = float((f_out[:B] - r_out).abs().max() / r_out.abs().max())
    print("logits: rel %.3e" % e)
    assert e <= 1e-5 and torch.equal(f_out[:B], f_out[B:])
    for n, a, b in zip(names, f_grads, r_grads):
        want = b if n == "x" else 2.0 * b                                 # a parameter's gradient is the sum over both ranks
        a = a[:B] if n == "x" else a
        e = float((a - want).abs().max() / want.abs().max())
        tol = 1e-5 if n in fp32 else 2.0 ** -7
        print("d %-30s rel %.3e (tolerance %.3e)" % (n, e, tol))
        assert e <= tol, n
    alone = _head(case, "hip", sd, 0.0)
    _run(alone, x, gout, names=names)
    for pre in ["psp_modules.%d.1.bn." % i for i in range(len(scales))] + ["bottleneck.bn."]:
        for stat in ("running_mean", "running_var"):
            a, b = rank.state_dict()[pre + stat], full.state_dict()[pre + stat]
            e = float((a - b).abs().max() / b.abs().max())
            print("%s%-12s two ranks vs concatenated: rel %.3e (tolerance 1e-5)" % (pre, stat, e))
            assert e <= 1e-5, pre + stat
        # the count went through the hook too: n / (n - 1) of twice the rows, not of one rank's
        assert float((rank.state_dict()[pre + "running_var"] - alone.state_dict()[pre + "running_var"]).abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------- with the loss
@pytest.mark.parametrize("case", ["P1", "P3"])
def test_forward_train_with_the_loss(case, monkeypatch):
    from mem_amd import ops
    B, Cin, C, K, h, w, scales = CASES[case]
    H, W = 16 * h, 16 * w
    x, sd, _ = state(case)
    lab = _labels(torch.Generator().manual_seed(5), B, K, H, W)
    p, lw = 0.1, 1.0
    keep = _mask(B, C, p).cpu()

    def expression(head_out, lab_long):
        up = F.interpolate(head_out, size=(H, W), mode="bilinear", align_corners=False)
        return lw * F.cross_entropy(up, lab_long, ignore_index=255, reduction="sum") / (B * H * W)

    ref = _head(case, "torch", sd, p, device="cpu", dtype=torch.float64)
    ref.keep_mask = keep
    x64 = x.double().requires_grad_()
    loss64 = expression(ref((x64,)), lab.long())
    loss64.backward()
    yard = _head(case, "torch", sd, p)
    yard.keep_mask = keep.cuda()
    xy = x.cuda().requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss_y = expression(yard((xy,)), lab.cuda().long())
    loss_y.float().backward()
    head = _head(case, "hip", sd, p)
    seen = {}
    real = ops.bnhead_bwd_sums

    def spy(dlogit, *a, **kw):
        seen["ops"] = (dlogit.data_ptr(), dlogit.stride())
        return real(dlogit, *a, **kw)

    monkeypatch.setattr(ops, "bnhead_bwd_sums", spy)
    xh = x.cuda().requires_grad_()
    logits = head((xh,))
    logits.register_hook(lambda g: seen.__setitem__("autograd", (g.data_ptr(), g.stride())))
    res = {"loss_seg": head.loss_decode(logits, lab.cuda()), "acc_seg": head.loss_decode.acc_seg()}
    res["loss_seg"].backward()
    figures = []
    ok = [held("loss_seg", res["loss_seg"], loss_y, loss64, figures), held("d map", xh.grad, xy.grad, x64.grad, figures)]
    report("%s with the loss" % case, figures)
    assert all(ok), [f for f, o in zip(figures, ok) if not o]
    print("dlogit as autograd delivered it", seen["autograd"], "as the kernel took it", seen["ops"])
    live = [i for i, n in enumerate(logits.shape) if n > 1]
    assert seen["ops"][0] == seen["autograd"][0]                          # pixel rows as the loss left them, no copy
    assert [seen["ops"][1][i] for i in live] == [seen["autograd"][1][i] for i in live] == [(h * w * K, 1, w * K, K)[i] for i in live]
    again = _head(case, "hip", sd, p)
    out = again.forward_train((x.cuda(),), lab.cuda())
    assert sorted(out) == ["acc_seg", "loss_seg"] and torch.equal(out["loss_seg"], res["loss_seg"].detach())
    up = F.interpolate(logits.detach().double().cpu(), size=(H, W), mode="bilinear", align_corners=False)
    valid = lab != 255
    n_correct = int(((up.argmax(1) == lab.long()) & valid).sum())
    stats = again.loss_decode.last_stats
    print("n_valid %d, n_correct %d (float64 on the head's logits: %d)" % (int(stats["n_valid"]), int(stats["n_correct"]), n_correct))
    assert int(stats["n_valid"]) == int(valid.sum()) and int(stats["n_correct"]) == n_correct
    assert float(out["acc_seg"]) == 100.0 * n_correct / int(valid.sum())


# ---------------------------------------------------------------------------------------------- through the backbone
CFG = dict(img_size=(112, 160), patch_size=16, in_chans=3, embed_dim=128, depth=4, num_heads=2, out_indices=(0, 1, 2, 3),
           use_rel_pos_bias=True, use_abs_pos_emb=False, init_values=0.1, drop_path_rate=0.0)


def _seg_model(impl, sd=None):
    from mem_amd.seg_heads import FCNHead, PSPHead, SegModel
    from mem_amd.semseg_backbone import EvBEiT
    from oracle.vit_ref import fill_by_name
    m = SegModel(EvBEiT(**CFG), PSPHead(128, 64, 11, in_index=2, impl=impl), auxiliary_head=FCNHead(128, 64, 11, in_index=2, impl=impl))
    if sd is None:
        trunk = {k: v for k, v in m.backbone.state_dict().items() if not k.startswith("fpn")}
        m.backbone.load_state_dict(fill_by_name(trunk, seed=5), strict=False)
        gen = torch.Generator().manual_seed(9)
        with torch.no_grad():
            for k, p in list(m.decode_head.named_parameters()) + list(m.auxiliary_head.named_parameters()):
                if k.endswith("conv.weight"):
                    p.copy_((torch.randn(p.shape, generator=gen) * (2.0 / (p.shape[1] * p.shape[2] * p.shape[3])) ** 0.5).to(torch.bfloat16).float())
                elif k == "conv_seg.weight":
                    p.copy_(torch.randn(p.shape, generator=gen) * 0.125)
        sd = {k: v.clone() for k, v in m.state_dict().items()}
    m.load_state_dict(sd, strict=True)
    m.decode_head.drop_key = m.auxiliary_head.drop_key = KEY
    return m.cuda().train(), sd


def _step(m, x, lab, autocast=False):
    """the trunk as it is, the (torch) heads alone under autocast; the loss is the sum of both heads'"""
    m.zero_grad(set_to_none=True)
    if autocast:
        feats = m.extract_feat(x)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = {"decode.loss_seg": m.decode_head.forward_train(feats, lab)["loss_seg"],
                   "aux.loss_seg": m.auxiliary_head.forward_train(feats, lab)["loss_seg"]}
    else:
        out = m.forward_train(x, lab)
    loss = out["decode.loss_seg"].float() + out["aux.loss_seg"].float()
    loss.backward()
    return loss.detach(), {k: p.grad.detach().float().clone() for k, p in m.named_parameters() if p.grad is not None}


def test_through_the_backbone():
    """SegModel(EvBEiT, PSPHead, FCNHead) with both heads hip: one forward_train + backward; trunk and head gradients against
    the same model with torch heads in fp32 (the reference here: there is no float64 trunk), held to the yardstick by torch heads
    under bf16 autocast behind the same trunk.  The three share the state dict and the Dropout2d masks."""
    from mem_amd import ops
    from oracle.gen_golden_ft import ft_inputs
    B = 4
    x = ft_inputs(dict(in_chans=3, img_size=(112, 160), num_classes=2), B, 3)[0].cuda()
    lab = _labels(torch.Generator().manual_seed(6), B, 11, 112, 160).cuda()
    mh, sd = _seg_model("hip")
    mt, _ = _seg_model("torch", sd)
    my, _ = _seg_model("torch", sd)
    assert (mh.decode_head.dropout_site, mh.auxiliary_head.dropout_site) == (ops.DROPOUT_SITE_HEAD, ops.DROPOUT_SITE_HEAD + 1)
    masks = []
    for i in range(2):
        keep = torch.empty((B, 64), dtype=torch.uint8, device="cuda")
        ops.dropout_mask(ops.dropout_params(KEY[0], KEY[1], ops.DROPOUT_SITE_HEAD + i, 0.1), 0, B, 64, keep)
        masks.append(keep)
    assert not torch.equal(masks[0], masks[1])                            # distinct sites: the heads draw different masks
    for m in (mt, my):
        m.decode_head.keep_mask, m.auxiliary_head.keep_mask = masks
    loss_h, g_h = _step(mh, x, lab)
    loss_t, g_t = _step(mt, x, lab)
    loss_y, g_y = _step(my, x, lab, autocast=True)
    trunk = [k for k, _ in mh.named_parameters() if k.startswith("backbone.") and not k.startswith("backbone.fpn")]
    heads = [k for k, _ in mh.named_parameters() if k.startswith(("decode_head.", "auxiliary_head."))]
    assert len(trunk) > 40 and len(heads) == 17 + 5
    for k in trunk + heads:
        assert (k in g_h or k not in g_t) and (k not in g_h or bool(torch.isfinite(g_h[k]).all())), k
    assert all(k in g_h for k in heads)
    pe = float(g_h["backbone.patch_embed.proj.weight"].abs().max())
    print("loss hip %.6f torch fp32 %.6f torch bf16 %.6f; |d patch_embed| max %.3e" % (float(loss_h), float(loss_t), float(loss_y), pe))
    assert pe > 0.0
    figures = []
    ok = [held("loss", loss_h, loss_y, loss_t, figures)]
    used = [k for k in trunk if k in g_t and float(g_t[k].abs().max()) > 0.0]          # blocks behind the exit of in_index = 2 get no gradient
    ok += [held("d " + k[len("backbone."):], g_h[k], g_y[k], g_t[k], figures) for k in used]
    ok += [held("d " + k, g_h[k], g_y[k], g_t[k], figures) for k in heads]
    report("through the backbone", figures)
    assert len(used) > 30 and all(ok), [f for f, o in zip(figures, ok) if not o]
    for k in trunk:
        if k not in used and k in g_h:
            assert float(g_h[k].abs().max()) == 0.0, k
