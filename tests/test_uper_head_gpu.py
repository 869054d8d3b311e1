"""-m gpu: the UPerNet decode head on the device.  The five FPN kernels each against float64 on the kernel's own stored inputs,
under bounds read off the code: an fp32 output is held to (its longest chain of fp32 roundings) x 2^-24 x (the sum of the
magnitudes of its terms), a bf16 output to 2^-8 relative in addition; a ReLU gate whose float64 pre-activation lies within fp32
rounding of zero may fall either way and its whole term joins the bounds it enters (tests/test_uper_head_cpu.py counts them).
Then UPerHead(impl="hip") forward and every gradient against the float64 torch arm fed the same bf16-valued maps, the same
weights and the same Dropout2d mask, under the project's yardstick:

    error(hip) <= 2 x error(torch arm under bf16 autocast on the GPU, same inputs) + 2^-20 x max |float64 result|

A quantity's error is its largest over four inputs per case (``SEEDS``), in either arm: on a single input the largest error of a
tensor is often one ReLU gate flipped by the bf16 rounding of a convolution output, and the ratio of the two arms' maxima
scatters beyond 2 in a third of the runs, for the merged ``PSPHead`` alone as for this head (``_against_reference``; DESIGN.md
section 2c, "UPerNet decode head", has the measurements)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from test_psp_head_gpu import SENTINEL, _padded_in, _padded_out, _ring_kept, _worst
from test_seg_head_gpu import KEY, _guarded, _guards_intact, _labels, _mask, held, report
from test_uper_head_cpu import CASES, U, bn_terms, kernel_inputs, param_names, state, table_pair

pytestmark = pytest.mark.gpu
KERNEL_CASES = ["U1", "U2", "U3", "U4", "BIG"]
HEAD_CASES = ["U1", "U2", "U3", "U4"]
SEEDS = (0, 1, 2, 3)          # the inputs of the whole-head yardstick: the first four states of every case


def _vectors(inp):
    return [inp[k].cuda() for k in ("mean", "rstd", "gamma", "beta")]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _relu_bn_fp32(inp, l):
    """bf16(relu(u)) as the kernels evaluate it, on the CPU: xhat = (y - mean) rstd in fp32 (two roundings), u one fused
    multiply-add (the exact product and sum in float64, rounded to fp32 once)"""
    y, m, rs = inp["Y"][l].float(), inp["mean"][l], inp["rstd"][l]
    xh = (y - m) * rs
    u = (xh.double() * inp["gamma"][l].double() + inp["beta"][l].double()).float()
    return u.clamp(min=0.0).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("case", KERNEL_CASES)
def test_topdown_fwd_against_float64(case):
    """T = bf16(relu(u) + bilinear(src)): u of the pixel 3 roundings (xhat 2, the fused multiply-add 1), the two weights 1 - w1
    one each, seven products and sums of the combination, the final sum: 13 behind the bf16 one when the source is a stored
    bf16 T; 3 more (u at the taps) when it is relu(bn(Y)) of the level above: 16 covers both.  The terms are those of u at the
    pixel plus the source's under the bilinear weights.  The forward is continuous in u: a gate at zero adds nothing."""
    from mem_amd import ops
    B, ins, C, K, sizes, scales = CASES[case]
    L = len(sizes)
    inp = kernel_inputs(case)
    vecs = _vectors(inp)
    print(case, "topdown_fwd")
    for l in range(L - 1):
        (h, w), My_Mx = sizes[l], table_pair(sizes[l + 1], sizes[l])
        My, Mx = My_Mx[:2]
        Y = _padded_in(inp["Y"][l])
        xh, u, mag_xh, mag_u, amb = bn_terms(inp, l)
        for mode in ["T"] + (["Y"] if l == L - 2 else []):
            if mode == "T":
                src = _padded_in(inp["T"][l + 1])
                s64, smag = inp["T"][l + 1].double(), inp["T"][l + 1].double().abs()
            else:
                src = (_padded_in(inp["Y"][l + 1]),)
                t = bn_terms(inp, l + 1)
                s64, smag = t[1].clamp(min=0.0), t[3]
            big, T = _padded_out(B, h, w, C)
            ops.fpn_topdown_fwd(l, sizes, Y, vecs, src, T)
            first = T.clone()
            assert _ring_kept(T) and _guards_intact(big)
            want = u.clamp(min=0.0) + torch.einsum("yi,bijc,xj->byxc", My, s64, Mx)
            mag = mag_u + torch.einsum("yi,bijc,xj->byxc", My, smag, Mx)
            err = (T[:, 1:-1, 1:-1].double().cpu() - want).abs()
            assert _worst("level %d <- %s" % (l, mode), err, 16 * U * mag + 2.0 ** -8 * want.abs()) <= 1.0
            T.fill_(SENTINEL)
            ops.fpn_topdown_fwd(l, sizes, Y, vecs, src, T)
            assert torch.equal(_bits(first), _bits(T))                            # two calls, the same bits


@pytest.mark.parametrize("case", KERNEL_CASES)
def test_concat_fwd_against_float64(case):
    """slice l: u at the four taps (3 roundings), the weights 1 - w1 (1 each), seven products and sums: 12 covers the chain
    behind the bf16 rounding; the terms are those of u at the taps under the bilinear weights.  Continuous in u.  A level of
    level 0's size (level 0 itself; every w1 == 0) holds bf16(relu(bn(Y))) bit for bit."""
    from mem_amd import ops
    B, ins, C, K, sizes, scales = CASES[case]
    L = len(sizes)
    inp = kernel_inputs(case)
    Y = [_padded_in(y) for y in inp["Y"]]
    big, xcat = _padded_out(B, sizes[0][0], sizes[0][1], L * C)
    ops.fpn_concat_fwd(sizes, Y, _vectors(inp), xcat)
    first = xcat.clone()
    assert _ring_kept(xcat) and _guards_intact(big)
    got = xcat[:, 1:-1, 1:-1].cpu()
    print(case, "concat_fwd")
    identities = 0
    for l in range(L):
        My, Mx, ty, tx = table_pair(sizes[l], sizes[0])
        xh, u, mag_xh, mag_u, amb = bn_terms(inp, l)
        want = torch.einsum("yi,bijc,xj->byxc", My, u.clamp(min=0.0), Mx)
        mag = torch.einsum("yi,bijc,xj->byxc", My, mag_u, Mx)
        sl = got[..., l * C:(l + 1) * C]
        assert _worst("level %d" % l, (sl.double() - want).abs(), 12 * U * mag + 2.0 ** -8 * want.abs()) <= 1.0
        if sizes[l] == sizes[0]:
            assert bool((ty[1] == 0).all()) and bool((tx[1] == 0).all())        # an identity table
            assert torch.equal(_bits(sl), _bits(_relu_bn_fp32(inp, l)))
            identities += 1
    assert identities >= 1
    xcat.fill_(SENTINEL)
    ops.fpn_concat_fwd(sizes, Y, _vectors(inp), xcat)
    assert torch.equal(_bits(first), _bits(xcat))


def _uses_of_resize_bwd(case):
    """(level, own?, slice of dxcat or None, fine rows?) of every use the head makes of the call"""
    L = len(CASES[case][4])
    uses = [(l, False, l, False) for l in range(L - 1)]                          # A_l
    uses += [(l, True, None, l > 0) for l in range(L - 1)]                       # dT_l, l < L - 1
    return uses + [(L - 1, False, L - 1, True)]                                  # dT_L-1


@pytest.mark.parametrize("case", KERNEL_CASES)
def test_resize_bwd_against_float64(case):
    """rows = own + gather(dxcat slice) + gather(fine rows): N = 1 + the (hi - lo + 1) of both axes of each source terms, each
    the product of two weights (1 - w1 and the sum of a clamped pair: 2 roundings) and one fused multiply-add: N + 4.  The own
    term alone (level 0 of the top-down backward) is the exact bf16 -> f32 conversion."""
    from mem_amd import ops
    B, ins, C, K, sizes, scales = CASES[case]
    L = len(sizes)
    inp = kernel_inputs(case)
    dxcat = _padded_in(inp["dxcat"])
    d64 = inp["dxcat"].double()
    print(case, "resize_bwd")
    exact = 0
    for l, has_own, sl, has_fine in _uses_of_resize_bwd(case):
        h, w = sizes[l]
        big, flat = _guarded(B * h * w * C, torch.float32)
        rows = flat.view(B * h * w, C)
        kw = {}
        want, mag = torch.zeros(B, h, w, C, dtype=torch.float64), torch.zeros(B, h, w, C, dtype=torch.float64)
        N = torch.zeros(h, w, dtype=torch.float64)
        if has_own:
            kw["own"] = _padded_in(inp["own"][l])
            want, mag, N = want + inp["own"][l].double(), mag + inp["own"][l].double().abs(), N + 1
        for src, n_out in ((d64[..., sl * C:(sl + 1) * C] if sl is not None else None, sizes[0]),
                           (inp["rows"][l - 1].double().view(B, *sizes[l - 1], C) if has_fine else None, sizes[l - 1] if l else None)):
            if src is None:
                continue
            My, Mx, ty, tx = table_pair(sizes[l], n_out)
            want = want + torch.einsum("yi,byxc,xj->bijc", My, src, Mx)
            mag = mag + torch.einsum("yi,byxc,xj->bijc", My, src.abs(), Mx)
            N = N + (torch.tensor(ty[3] - ty[2] + 1)[:, None] * torch.tensor(tx[3] - tx[2] + 1)[None, :]).double()
        if sl is not None:
            kw.update(dxcat=dxcat, slice_=sl)
        if has_fine:
            kw["fine_rows"] = inp["rows"][l - 1].cuda()
        ops.fpn_resize_bwd(l, sizes, C, rows, **kw)
        first = rows.clone()
        assert _guards_intact(big)
        err = (rows.double().cpu().view(B, h, w, C) - want).abs()
        name = "level %d%s%s%s (at most %d terms)" % (l, " own" if has_own else "", " dxcat[%d]" % sl if sl is not None else "",
                                                      " fine" if has_fine else "", int(N.max()))
        assert _worst(name, err, (N[None, :, :, None] + 4) * U * mag) <= 1.0
        if has_own and sl is None and not has_fine:
            assert torch.equal(rows.cpu().view(B, h, w, C), inp["own"][l].float())
            exact += 1
        flat.fill_(float("nan"))
        ops.fpn_resize_bwd(l, sizes, C, rows, **kw)
        assert torch.equal(first, rows)
    assert exact == 1


def _sums_chain(R):
    """the longest chain of fp32 roundings behind a channel sum over R rows: a row lane's chain, the 32 lanes, the G partials"""
    G = min(-(-R // 32), 128)
    return -(-R // (32 * G)) + 32 + G


@pytest.mark.parametrize("case", KERNEL_CASES)
def test_bn_bwd_sums_against_float64(case):
    """sums = sum g, sum g xhat, g = rows (u > 0): the chain of the two-stage sum (ceil(R / (32 G)) + 32 + G), and 4 more for
    xhat and its product.  An ambiguous gate's |rows| joins the bounds."""
    from mem_amd import ops
    B, ins, C, K, sizes, scales = CASES[case]
    inp = kernel_inputs(case)
    vecs = _vectors(inp)
    ws = ops.fpn_sums_workspace(C, "cuda")
    print(case, "bn_bwd_sums")
    n_amb = n_all = 0
    for l, (h, w) in enumerate(sizes):
        R = B * h * w
        Y, rows = _padded_in(inp["Y"][l]), inp["rows"][l].cuda()
        big, flat = _guarded(2 * C, torch.float32)
        sums = flat.view(2, C)
        ws.fill_(float("nan"))
        ops.fpn_bn_bwd_sums(l, sizes, Y, vecs, rows, sums, ws)
        first = sums.clone()
        assert _guards_intact(big)
        xh, u, mag_xh, mag_u, amb = bn_terms(inp, l)
        r64 = inp["rows"][l].double().view(B, h, w, C)
        g = r64 * (u > 0)
        slack = amb * r64.abs()
        Lc = _sums_chain(R)
        want = torch.stack([g.sum((0, 1, 2)), (g * xh).sum((0, 1, 2))])
        bound = torch.stack([Lc * U * g.abs().sum((0, 1, 2)) + slack.sum((0, 1, 2)),
                             (Lc + 4) * U * (g.abs() * mag_xh).sum((0, 1, 2)) + (slack * mag_xh).sum((0, 1, 2))])
        assert _worst("level %d (chain %d)" % (l, Lc), (sums.double().cpu() - want).abs(), bound) <= 1.0
        n_amb, n_all = n_amb + int(amb.sum()), n_all + amb.numel()
        flat.fill_(float("nan"))
        ws.fill_(0.0)                                                             # whatever the workspace held
        ops.fpn_bn_bwd_sums(l, sizes, Y, vecs, rows, sums, ws)
        assert torch.equal(first, sums)
    print("    %d of %d gates within fp32 rounding of zero" % (n_amb, n_all))
    assert n_amb <= 1e-3 * n_all


@pytest.mark.parametrize("case", KERNEL_CASES)
def test_bn_bwd_apply_against_float64(case):
    """gamma rstd (g - tot0 inv_n - xhat tot1 inv_n): ten roundings at most behind the bf16 one; tot None: no correction terms.
    An ambiguous gate's gamma rstd |rows| joins the bound."""
    from mem_amd import ops
    B, ins, C, K, sizes, scales = CASES[case]
    inp = kernel_inputs(case)
    vecs = _vectors(inp)
    print(case, "bn_bwd_apply")
    for l, (h, w) in enumerate(sizes):
        Y, rows = _padded_in(inp["Y"][l]), inp["rows"][l].cuda()
        xh, u, mag_xh, mag_u, amb = bn_terms(inp, l)
        r64 = inp["rows"][l].double().view(B, h, w, C)
        g = r64 * (u > 0)
        sc = inp["gamma"][l].double() * inp["rstd"][l].double()
        for tot in (inp["tot"], None):
            big, dY = _padded_out(B, h, w, C)
            ops.fpn_bn_bwd_apply(l, sizes, Y, vecs, rows, None if tot is None else tot.cuda(), inp["inv_n"][l], dY)
            t0, t1 = (0.0, 0.0) if tot is None else (tot[0].double() * inp["inv_n"][l], tot[1].double() * inp["inv_n"][l])
            t0a, t1a = (0.0, 0.0) if tot is None else (t0.abs(), t1.abs())
            want = sc * (g - t0 - xh * t1)
            bound = 2.0 ** -8 * want.abs() + 10 * U * sc.abs() * (g.abs() + t0a + mag_xh * t1a) + amb * sc.abs() * r64.abs() * (1 + 2.0 ** -8)
            err = (dY[:, 1:-1, 1:-1].double().cpu() - want).abs()
            assert _worst("level %d%s" % (l, "" if tot is not None else " eval"), err, bound) <= 1.0
            assert _ring_kept(dY) and _guards_intact(big)
        big2, again = _padded_out(B, h, w, C)
        ops.fpn_bn_bwd_apply(l, sizes, Y, vecs, rows, None, inp["inv_n"][l], again)
        assert torch.equal(_bits(dY), _bits(again))


# ---------------------------------------------------------------------------------------------- the head against float64
def _names(case):
    B, ins, C, K, sizes, scales = CASES[case]
    return ["x%d" % l for l in range(len(ins))] + param_names(len(ins), len(scales))


def _head(case, impl, sd, p, train=True, device="cuda", dtype=None):
    from mem_amd.seg_heads import UPerHead
    B, ins, C, K, sizes, scales = CASES[case]
    head = UPerHead(in_channels=ins, channels=C, num_classes=K, in_index=tuple(range(len(ins))), pool_scales=scales, dropout_ratio=p,
                    impl=impl)
    head.load_state_dict(sd, strict=True)
    head.drop_key = KEY
    if dtype is not None:
        head = head.to(dtype)
    return head.to(device).train(train)


def _run(head, xs, gout, autocast=False, names=None):
    """logits and the gradients of one forward + backward, on the head's device"""
    dev, L = head.conv_seg.weight.device, len(xs)
    head.zero_grad(set_to_none=True)
    xg = [x.to(dev, head.conv_seg.weight.dtype).requires_grad_() for x in xs]
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        out = head(tuple(xg))
    if out.dtype == torch.float64:
        out.backward(gout.to(dev, torch.float64))
    else:
        out.float().backward(gout.to(dev))
    ps = dict(head.named_parameters())
    grads = [x.grad for x in xg] + [ps[n].grad for n in names[L:]]
    return out.detach().clone(), [g.detach().clone() for g in grads]


@functools.lru_cache(maxsize=None)
def _reference(case, p, train=True, seed=0):
    """the torch arm in float64 on the CPU, once per (case, seed): logits and gradients, with the mask of the contract"""
    B, ins, C, K, sizes, scales = CASES[case]
    xs, sd, gout = state(case, seed)
    keep = _mask(B, C, p).cpu() if (train and p > 0.0) else None
    ref = _head(case, "torch", sd, p, train, device="cpu", dtype=torch.float64)
    ref.keep_mask = keep
    out, grads = _run(ref, xs, gout, names=_names(case))
    return out, grads, keep


def _pool(worst, figures):
    """fold one input's figures (name, error hip, error yardstick, bound) into the largest errors per quantity over the inputs;
    the third entry is the bound's floor, 2^-20 max |reference|"""
    for name, e_got, e_yard, bound in figures:
        w = worst.setdefault(name, [0.0, 0.0, 0.0])
        w[0], w[1], w[2] = max(w[0], e_got), max(w[1], e_yard), max(w[2], bound - 2.0 * e_yard)


def _pooled(worst):
    return [(name, w[0], w[1], 2.0 * w[1] + w[2]) for name, w in worst.items()]


def _against_reference(case, p, train=True):
    """The yardstick over the inputs of SEEDS, per quantity: its error is its largest error over those inputs, in either arm
    (the issue's formula, on a sample of four inputs in place of one).  One input does not do: the largest error of a tensor
    is often ONE ReLU gate that bf16 rounding of a convolution output flips, in either arm (at U2 / seed 4 both arms flip 3 of
    the inner bottleneck's 5 760 gates; the hip arm's third carries 4 x the median gradient and is 30 of its 30 units of error
    in ``bottleneck.conv.weight``, every other row being 4.9 against autocast's 3.5), so that on single inputs the ratio of the
    two arms' maxima exceeds 2 in a third of the runs -- for the merged ``PSPHead`` alone just as for this head (DESIGN.md
    section 2c has the figures).  Returns the verdicts, the pooled figures (name, error hip, error yardstick, bound) and the
    geometric mean over the quantities of error(hip) / error(yardstick) per input."""
    names = _names(case)
    worst, geo = {}, []
    for seed in SEEDS:
        xs, sd, gout = state(case, seed)
        ref_out, ref_grads, keep = _reference(case, p, train, seed)
        hip_out, hip_grads = _run(_head(case, "hip", sd, p, train), xs, gout, names=names)
        yard = _head(case, "torch", sd, p, train)
        yard.keep_mask = None if keep is None else keep.cuda()
        yard_out, yard_grads = _run(yard, xs, gout, autocast=True, names=names)
        figures = []
        held("logits", hip_out, yard_out, ref_out, figures)
        for n, a, b, c in zip(names, hip_grads, yard_grads, ref_grads):
            held("d " + n, a, b, c, figures)
        report("%s p=%.1f %s seed %d" % (case, p, "train" if train else "eval", seed), figures)
        ratios = [f[1] / f[2] for f in figures if f[1] > 0.0 and f[2] > 0.0]
        geo.append(math.exp(sum(math.log(r) for r in ratios) / len(ratios)))
        _pool(worst, figures)
    pooled = _pooled(worst)
    report("%s p=%.1f %s over seeds %s" % (case, p, "train" if train else "eval", list(SEEDS)), pooled)
    top = max(pooled, key=lambda f: f[1] / max(f[3], 1e-300))
    print("%s largest error / bound over the seeds %.3f (%s); geometric mean of error(hip) / error(yardstick) per seed: %s"
          % (case, top[1] / max(top[3], 1e-300), top[0], ["%.2f" % g for g in geo]))
    return [f[1] <= f[3] for f in pooled], pooled, geo


@pytest.mark.parametrize("case", HEAD_CASES)
def test_forward_and_backward_within_twice_torchs_own_error(case):
    ok, figures, geo = _against_reference(case, 0.1)
    assert all(ok), [f for f, o in zip(figures, ok) if not o]


def test_two_calls_give_the_same_bits():
    case = "U2"
    xs, sd, gout = state(case)
    head = _head(case, "hip", sd, 0.1)
    a_out, a_grads = _run(head, xs, gout, names=_names(case))
    b_out, b_grads = _run(head, xs, gout, names=_names(case))
    assert torch.equal(a_out, b_out) and all(torch.equal(a, b) for a, b in zip(a_grads, b_grads))
    assert all(bool(torch.isfinite(g).all()) for g in a_grads) and bool(torch.isfinite(a_out).all())


def _forward_buffers(L, n):
    return sorted(["logits", "xcat", "y", "psp.xcat", "psp.y"] + ["ppm.p%d" % i for i in range(n)] + ["ppm.y%d" % i for i in range(n)]
                  + [pre % l for l in range(L - 1) for pre in ("lat.xp%d", "lat.y%d", "fpn.t%d", "fpn.y%d")]
                  + ["%s.vec.%s" % (a, k) for a in ("lat", "fpn") for k in ("mean", "rstd", "gamma", "beta")])


def test_eval_mode_uses_the_running_statistics_and_changes_none():
    case = "U1"
    B, ins, C, K, sizes, scales = CASES[case]
    L, n = len(ins), len(scales)
    xs, sd, gout = state(case)
    ok, figures, geo = _against_reference(case, 0.1, train=False)
    assert all(ok), [f for f, o in zip(figures, ok) if not o]
    head = _head(case, "hip", sd, 0.1, train=False)
    with torch.no_grad():
        out = head(tuple(x.cuda() for x in xs))
    ref_out = _reference(case, 0.1, False)[0]
    print("eval, no_grad: max error %.3e" % float((out.double().cpu() - ref_out).abs().max()))
    assert not out.requires_grad and float((out.double().cpu() - ref_out).abs().max()) <= 2.0 ** -7 * float(ref_out.abs().max())
    now = head.state_dict()
    stats = [k for k in sd if "running_" in k or "num_batches" in k]
    assert len(stats) == 3 * (2 * L + n) and all(torch.equal(now[k].cpu(), sd[k]) for k in stats)
    used = sorted(k[0] for k in head._bufs)
    print("buffers of an eval forward under no_grad:", used)
    assert used == _forward_buffers(L, n)                                         # eval statistics: no sums, no workspaces
    head.train()
    head(tuple(x.cuda().requires_grad_() for x in xs))
    now = head.state_dict()
    assert all(int(now[k]) == 4 for k in stats if "num_batches" in k)
    assert not any(torch.equal(now[k].cpu(), sd[k]) for k in stats if "running_" in k)


def test_running_statistics_match_batchnorm():
    """two training forwards: the running statistics of all 2 L + n batch norms of the hip arm against torch's batch norm in
    float64 (the torch arm, on the same maps): fp32 statistics of bf16-rounded values, 2^-9 relative on every value at most, so
    2^-8 of the spread is ample (tests/test_psp_head_gpu.py's tolerance and argument)"""
    case = "U2"
    B, ins, C, K, sizes, scales = CASES[case]
    xs, sd, gout = state(case)
    head = _head(case, "hip", sd, 0.1)
    ref = _head(case, "torch", sd, 0.0, device="cpu", dtype=torch.float64)
    for i in range(2):
        xi = [(x * (1.0 + i)).to(torch.bfloat16).float() for x in xs]
        with torch.no_grad():
            head(tuple(x.cuda() for x in xi))
            ref(tuple(x.double() for x in xi))
    got, want = head.state_dict(), ref.state_dict()
    pres = sorted(k[:-len("running_mean")] for k in sd if k.endswith("running_mean"))
    assert len(pres) == 2 * len(ins) + len(scales)
    for pre in pres:
        em = float((got[pre + "running_mean"].double().cpu() - want[pre + "running_mean"]).abs().max())
        ev = float((got[pre + "running_var"].double().cpu() - want[pre + "running_var"]).abs().max())
        print("%-26s running mean error %.3e, running var error %.3e" % (pre, em, ev))
        assert int(got[pre + "num_batches_tracked"]) == 5 == int(want[pre + "num_batches_tracked"])
        assert em <= 2.0 ** -8 * float(want[pre + "running_var"].sqrt().max()) and ev <= 2.0 ** -8 * float(want[pre + "running_var"].max())


def test_a_second_step_sees_the_optimizers_weights():
    """the bf16 weight copies follow torch's version counter: after optimizer.step() the next forward is that of a fresh head
    holding the new state dict, bit for bit, and not the first step's"""
    case = "U1"
    xs, sd, gout = state(case)
    names = _names(case)
    head = _head(case, "hip", sd, 0.1)
    opt = torch.optim.SGD(head.parameters(), lr=0.01)
    out1, _ = _run(head, xs, gout, names=names)
    opt.step()
    out2, grads2 = _run(head, xs, gout, names=names)
    fresh = _head(case, "hip", {k: v.detach().cpu().clone() for k, v in head.state_dict().items()}, 0.1)
    out3, grads3 = _run(fresh, xs, gout, names=names)
    moved = float((out2 - out1).abs().max())
    print("the step moved the logits by %.3e" % moved)
    assert moved > 1e-3 and torch.equal(out2, out3) and all(torch.equal(a, b) for a, b in zip(grads2, grads3))


# ---------------------------------------------------------------------------------------------- SyncBN hook
def test_syncbn_hook_two_identical_ranks():
    """reduce doubles the sums (two ranks holding the same batch): the result is the single-rank run on the batch
    concatenated with itself, and the exchanges are the nine of the head's docstring, in order.  PSPHead's test and its two
    tolerances: the statistics of the two runs are added in different orders (relative differences of a few 2^-24 on mean and
    rstd), so fp32 results -- the logits, the gradients of fpn_bottleneck's batch norm and of conv_seg, every running statistic
    -- agree to 1e-5 of their largest value; what passes a bf16 gradient, where such a difference can move single elements by
    one bf16 step (2^-8 relative), agrees to 2^-7."""
    case = "U2"
    B, ins, C, K, sizes, scales = CASES[case]
    L = len(ins)
    xs, sd, gout = state(case)
    names = _names(case)
    calls = []

    def doubled(vec, tag):
        calls.append((tag, tuple(vec.shape)))
        return vec * 2.0

    rank = _head(case, "hip", sd, 0.0)
    rank.reduce = doubled
    r_out, r_grads = _run(rank, xs, gout, names=names)
    full = _head(case, "hip", sd, 0.0)
    f_out, f_grads = _run(full, [torch.cat([x, x]) for x in xs], torch.cat([gout, gout]), names=names)
    n = len(scales)
    print(calls)
    assert calls == [("stats", (L - 1, 3, C)), ("stats", (n, 3, C)), ("stats", (3, C)), ("stats", (L - 1, 3, C)), ("stats", (3, C)),
                     ("bwd", (2, C)), ("bwd", (L - 1, 2, C)), ("bwd", (L, 2, C)), ("bwd", (n, 2, C))]
    fp32 = {"fpn_bottleneck.bn.weight", "fpn_bottleneck.bn.bias", "conv_seg.weight", "conv_seg.bias"}
    e = float((f_out[:B] - r_out).abs().max() / r_out.abs().max())
    print("logits: rel %.3e" % e)
    assert e <= 1e-5 and torch.equal(f_out[:B], f_out[B:])
    for nm, a, b in zip(names, f_grads, r_grads):
        is_map = nm.startswith("x")
        want = b if is_map else 2.0 * b                                   # a parameter's gradient is the sum over both ranks
        a = a[:B] if is_map else a
        e = float((a - want).abs().max() / want.abs().max())
        tol = 1e-5 if nm in fp32 else 2.0 ** -7
        print("d %-32s rel %.3e (tolerance %.3e)" % (nm, e, tol))
        assert e <= tol, nm
    alone = _head(case, "hip", sd, 0.0)
    _run(alone, xs, gout, names=names)
    for pre in sorted(k[:-len("running_mean")] for k in sd if k.endswith("running_mean")):
        for stat in ("running_mean", "running_var"):
            a, b = rank.state_dict()[pre + stat], full.state_dict()[pre + stat]
            e = float((a - b).abs().max() / b.abs().max())
            print("%s%-12s two ranks vs concatenated: rel %.3e (tolerance 1e-5)" % (pre, stat, e))
            assert e <= 1e-5, pre + stat
        # the count went through the hook too: n / (n - 1) of twice the rows, not of one rank's
        assert float((rank.state_dict()[pre + "running_var"] - alone.state_dict()[pre + "running_var"]).abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------- with the loss
def test_forward_train_with_the_loss(monkeypatch):
    """loss and map gradients under the yardstick over the inputs of SEEDS (``_against_reference`` says why); at seed 0 also:
    ``dlogit`` reaches the tail as the loss left it, ``forward_train``'s result, and the counts of ``acc_seg``"""
    from mem_amd import ops
    case = "U1"
    B, ins, C, K, sizes, scales = CASES[case]
    h, w = sizes[0]
    H, W = 4 * h, 4 * w
    lab = _labels(torch.Generator().manual_seed(5), B, K, H, W)
    p, lw = 0.1, 1.0
    keep = _mask(B, C, p).cpu()

    def expression(head_out, lab_long):
        up = F.interpolate(head_out, size=(H, W), mode="bilinear", align_corners=False)
        return lw * F.cross_entropy(up, lab_long, ignore_index=255, reduction="sum") / (B * H * W)

    seen = {}
    real = ops.bnhead_bwd_sums

    def spy(dlogit, *a, **kw):
        seen["ops"] = (dlogit.data_ptr(), dlogit.stride())
        return real(dlogit, *a, **kw)

    monkeypatch.setattr(ops, "bnhead_bwd_sums", spy)
    worst, first = {}, None
    for seed in SEEDS:
        xs, sd, _ = state(case, seed)
        ref = _head(case, "torch", sd, p, device="cpu", dtype=torch.float64)
        ref.keep_mask = keep
        x64 = [x.double().requires_grad_() for x in xs]
        loss64 = expression(ref(tuple(x64)), lab.long())
        loss64.backward()
        yard = _head(case, "torch", sd, p)
        yard.keep_mask = keep.cuda()
        xy = [x.cuda().requires_grad_() for x in xs]
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss_y = expression(yard(tuple(xy)), lab.cuda().long())
        loss_y.float().backward()
        head = _head(case, "hip", sd, p)
        xh = [x.cuda().requires_grad_() for x in xs]
        logits = head(tuple(xh))
        logits.register_hook(lambda g: seen.__setitem__("autograd", (g.data_ptr(), g.stride())))
        res = {"loss_seg": head.loss_decode(logits, lab.cuda()), "acc_seg": head.loss_decode.acc_seg()}
        res["loss_seg"].backward()
        figures = []
        held("loss_seg", res["loss_seg"], loss_y, loss64, figures)
        for l, (a, b, c) in enumerate(zip(xh, xy, x64)):
            held("d map %d" % l, a.grad, b.grad, c.grad, figures)
        report("%s with the loss, seed %d" % (case, seed), figures)
        _pool(worst, figures)
        if first is None:
            first = (xs, sd, logits.detach(), res["loss_seg"].detach(), dict(seen))
    pooled = _pooled(worst)
    report("%s with the loss over seeds %s" % (case, list(SEEDS)), pooled)
    assert all(f[1] <= f[3] for f in pooled), [f for f in pooled if f[1] > f[3]]
    xs, sd, logits, loss_seg, seen = first
    print("dlogit as autograd delivered it", seen["autograd"], "as the kernel took it", seen["ops"])
    live = [i for i, n in enumerate(logits.shape) if n > 1]
    assert seen["ops"][0] == seen["autograd"][0]                          # pixel rows as the loss left them, no copy
    assert [seen["ops"][1][i] for i in live] == [seen["autograd"][1][i] for i in live] == [(h * w * K, 1, w * K, K)[i] for i in live]
    again = _head(case, "hip", sd, p)
    out = again.forward_train(tuple(x.cuda() for x in xs), lab.cuda())
    assert sorted(out) == ["acc_seg", "loss_seg"] and torch.equal(out["loss_seg"], loss_seg)
    up = F.interpolate(logits.double().cpu(), size=(H, W), mode="bilinear", align_corners=False)
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
    from mem_amd.seg_heads import FCNHead, SegModel, UPerHead
    from mem_amd.semseg_backbone import EvBEiT
    from oracle.vit_ref import fill_by_name
    m = SegModel(EvBEiT(**CFG), UPerHead((128,) * 4, 64, 11, pool_scales=(1, 2, 3), impl=impl),
                 auxiliary_head=FCNHead(128, 64, 11, in_index=2, impl=impl))
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


def test_through_the_backbone():
    """SegModel(EvBEiT, UPerHead, FCNHead) with both heads hip: one forward_train + backward; trunk and head gradients against
    the same model with torch heads in fp32 (the reference here: there is no float64 trunk), held to the yardstick by torch heads
    under bf16 autocast behind the same trunk.  The three share the state dict and the Dropout2d masks.  The decode head reads
    every exit, so every block of the trunk receives gradient.

    A quantity's error is its largest over four inputs, in either arm (``_against_reference`` says why), each input on fresh
    models (the engine keeps gradient buffers between steps).  Here no arm repeats its bits between two runs -- the trunk's
    backward and torch's resize / pooling backward add in an order that varies -- and on one input a single tensor's
    error / bound moved by up to 0.44 between two runs (``blocks.3.mlp.fc2.bias`` 0.90 / 0.45; largest over the tensors 0.64 .. 0.90
    over 6 inputs x 2 runs, all within the bound); over the four inputs the largest was 0.79 .. 0.80 in all 16 combinations of those runs."""
    from mem_amd import ops
    from oracle.gen_golden_ft import ft_inputs
    from test_psp_head_gpu import _step
    B = 4
    _, sd = _seg_model("hip")
    masks = []
    for i in range(2):
        keep = torch.empty((B, 64), dtype=torch.uint8, device="cuda")
        ops.dropout_mask(ops.dropout_params(KEY[0], KEY[1], ops.DROPOUT_SITE_HEAD + i, 0.1), 0, B, 64, keep)
        masks.append(keep)
    assert not torch.equal(masks[0], masks[1])                            # distinct sites: the heads draw different masks
    worst = {}
    for k in range(4):
        x = ft_inputs(dict(in_chans=3, img_size=(112, 160), num_classes=2), B, 3 + k)[0].cuda()
        lab = _labels(torch.Generator().manual_seed(6 + k), B, 11, 112, 160).cuda()
        mh, _ = _seg_model("hip", sd)
        mt, _ = _seg_model("torch", sd)
        my, _ = _seg_model("torch", sd)
        if k == 0:
            with torch.no_grad():
                assert [tuple(f.shape[2:]) for f in mh.extract_feat(x)] == [(28, 40), (14, 20), (7, 10), (3, 5)]
        for m in (mt, my):
            m.decode_head.keep_mask, m.auxiliary_head.keep_mask = masks
        loss_h, g_h = _step(mh, x, lab)
        loss_t, g_t = _step(mt, x, lab)
        loss_y, g_y = _step(my, x, lab, autocast=True)
        trunk = [n for n, _ in mh.named_parameters() if n.startswith("backbone.") and not n.startswith("backbone.fpn")]
        heads = [n for n, _ in mh.named_parameters() if n.startswith(("decode_head.", "auxiliary_head."))]
        assert len(trunk) > 40 and len(heads) == 35 + 5
        assert all(n in g_h and bool(torch.isfinite(g_h[n]).all()) for n in heads)
        print("input %d: loss hip %.6f torch fp32 %.6f torch bf16 %.6f" % (k, float(loss_h), float(loss_t), float(loss_y)))
        figures = []
        held("loss", loss_h, loss_y, loss_t, figures)
        used = [n for n in trunk if n in g_t and float(g_t[n].abs().max()) > 0.0]
        for n in used:
            held("d " + n[len("backbone."):], g_h[n], g_y[n], g_t[n], figures)
        for n in heads:
            held("d " + n, g_h[n], g_y[n], g_t[n], figures)
        report("through the backbone, input %d" % k, figures)
        _pool(worst, figures)
        # the blocks behind every exit receive gradient now: no used trunk parameter is left at zero
        assert len(used) > 40 and any(n.startswith("backbone.blocks.3.") for n in used)
        for n in used:
            assert n in g_h and bool(torch.isfinite(g_h[n]).all()) and float(g_h[n].abs().max()) > 0.0, n
        del mh, mt, my
    pooled = _pooled(worst)
    report("through the backbone over 4 inputs", pooled)
    top = max(pooled, key=lambda f: f[1] / max(f[3], 1e-300))
    print("largest error / bound over the inputs %.3f (%s)" % (top[1] / max(top[3], 1e-300), top[0]))
    assert all(f[1] <= f[3] for f in pooled), [f for f in pooled if f[1] > f[3]]


# ---------------------------------------------------------------------------------------------- loading
def test_a_reference_state_dict_loads_strictly_and_the_pyramid_moves_from_a_psp_head():
    from mem_amd.seg_heads import PSPHead
    from test_uper_head_cpu import dims_of, mmseg_keys
    case = "U1"
    B, ins, C, K, sizes, scales = CASES[case]
    xs, sd, gout = state(case)
    dims = dims_of(case)
    built = {k: torch.zeros(tuple(dims.get(d, d) for d in shape), dtype=torch.long if k.endswith("tracked") else torch.float32)
             for k, shape in mmseg_keys(len(ins), len(scales)).items()}
    _head(case, "hip", built, 0.1)                                        # strict=True inside
    psp = PSPHead(in_channels=ins[-1], channels=C, num_classes=K, in_index=0, pool_scales=scales, impl="hip")
    psp.load_state_dict({k: v for k, v in sd.items() if k.startswith(("psp_modules.", "bottleneck.", "conv_seg."))}, strict=True)
    head = _head(case, "hip", built, 0.1)
    mine = {k: v for k, v in psp.state_dict().items() if k.startswith(("psp_modules.", "bottleneck."))}
    missing, unexpected = head.load_state_dict(mine, strict=False)
    assert not unexpected and all(not k.startswith(("psp_modules.", "bottleneck.")) for k in missing)
    assert all(torch.equal(head.state_dict()[k].cpu(), sd[k]) for k in mine)
