"""-m gpu: the fused feature-pyramid necks on the device -- the movement kernels of csrc/necks.hip bit-exact against the
torch expressions that specify them (mem_amd.necks.map_to_rows / rows_to_map), the two-stage column statistics against
float64 under a bound derived from their summation structure, fpn1 / fpn2 forward and backward against float64 on the CPU
fed the same bf16-rounded map and weights, the batch-norm bookkeeping, the SyncBN algebra through a replaced reduce function,
and EvBEiT(necks="fused") end to end.

Measured on MI355X (relative L2 per map against float64; fused | torch modules under bf16 autocast):
  see DESIGN.md section 2c, "Feature-pyramid necks"."""
import contextlib
import io

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (B, D, Hp, Wp): ragged against the 64-tiles; row lengths 35 / 14 that are no multiple of 4 and D no multiple of 128; the
# real width (GEMM N = 3072, up to 6272 rows)
SHAPES = [(3, 128, 4, 6), (1, 192, 5, 7), (2, 768, 14, 14)]
GUARD = 256
U = 2.0 ** -24           # unit roundoff of fp32
FWD_BAR = 2.0 ** -8      # per bf16 rounding of the fused path behind the shared ones (2^-9 relative each, doubled)


def _guarded(n, dtype):
    big = torch.full((n + 2 * GUARD,), float("nan"), device="cuda", dtype=dtype)
    return big, big[GUARD:GUARD + n]


def _guards_intact(big):
    return bool(torch.isnan(big[:GUARD]).all() and torch.isnan(big[-GUARD:]).all())


# ---------------------------------------------------------------------------------------------- layout kernels
@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("B,D,Hp,Wp", SHAPES)
def test_maps_to_rows_bit_exact(B, D, Hp, Wp, level):
    from mem_amd import necks as N, ops
    g = torch.Generator().manual_seed(B * 1000 + D + Hp * Wp + level)
    x = torch.randn((B, D, Hp << level, Wp << level), generator=g).cuda()
    want = N.map_to_rows(x, level).to(torch.bfloat16)                            # one round-to-nearest-even
    big, out = _guarded(want.numel(), torch.bfloat16)
    got = ops.neck_maps_to_rows(x, level, out=out.view(want.shape))
    assert torch.equal(got.view(torch.int16), want.contiguous().view(torch.int16))
    assert _guards_intact(big)


@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("B,D,Hp,Wp", SHAPES)
def test_rows_to_maps_bit_exact(B, D, Hp, Wp, level):
    from mem_amd import necks as N, ops
    g = torch.Generator().manual_seed(B * 1000 + D + Hp * Wp + level + 7)
    R0 = B * Hp * Wp
    shape = (R0, D) if level == 0 else (R0 * 4 ** (level - 1), 4 * D)
    rows = torch.randn(shape, generator=g).to(torch.bfloat16).cuda()
    want = N.rows_to_map(rows, B, D, Hp, Wp, level).float().contiguous()
    big, out = _guarded(want.numel(), torch.float32)
    got = ops.neck_rows_to_maps(rows, B, D, Hp, Wp, level, out=out.view(want.shape))
    assert torch.equal(got, want)
    assert _guards_intact(big)
    back = ops.neck_maps_to_rows(got, level)                                      # and the round trip is the identity
    assert torch.equal(back.view(torch.int16), rows.view(torch.int16))


# ---------------------------------------------------------------------------------------------- statistics
def _chain(R):
    """The longest chain of fp32 additions behind one output of memhip_neck_colstats (include/memhip.h): a thread adds its
    4 values of each of ceil(R / (8 G)) rows one after the other, 8 thread partials are folded in order, then the G
    workgroup partials."""
    from mem_amd import ops
    G = min(-(-R // 8), ops.NECK_GROUPS)
    return 4 * -(-R // (8 * G)) + 8 + G


@pytest.mark.parametrize("offset", [0.0, 1e3])
@pytest.mark.parametrize("B,D,Hp,Wp", SHAPES)
def test_colstats_against_float64(B, D, Hp, Wp, offset):
    """count, sum (x - s), sum (x - s)^2 per channel over [R, 4D] interleaved against float64 on the same bf16 values and
    fp32 shift.  Bounds from the summation structure (first order in u = 2^-24, times 1.01 for the higher orders):
      |sum1 - ref|  <=  (chain + 1) u sum |x - s|        (+ 1: the rounding of x - s itself)
      |sum2 - ref|  <=  (chain + 3) u sum (x - s)^2      (+ 2 more: the square of a rounded difference)
    and for what the batch norm derives from them, mean = s + sum1 / n and var = sum2 / n - (sum1 / n)^2:
      |var - ref|   <=  u ((chain + 3) E(x - s)^2 + 2 |E(x - s)| (chain + 1) E|x - s|)
    N(0, 1) data, and the same data on a common offset of 1e3 with the shift near it: the statistics survive the offset
    (var = E[x^2] - mean^2 on raw fp32 sums would carry an error of 1e6 u = 0.06 into a variance of about 2)."""
    from mem_amd import ops
    R = B * Hp * Wp
    g = torch.Generator().manual_seed(R + D)
    y = (torch.randn((R, 4 * D), generator=g) + offset).to(torch.bfloat16).cuda()
    s = (offset + 0.02 * torch.randn(D, generator=g)).float().cuda()
    ws = ops.neck_sums_workspace(D, "cuda")
    big, out = _guarded(3 * D, torch.float32)
    st = ops.neck_colstats(y, s, ws, out=out.view(3, D)).double().cpu()
    assert _guards_intact(big)
    d = y.double().cpu().view(R, D, 4) - s.double().cpu().view(1, D, 1)          # [R, D, q]
    n = 4 * R
    ref1, ref2, abs1 = d.sum((0, 2)), (d * d).sum((0, 2)), d.abs().sum((0, 2))
    chain = _chain(R)
    assert torch.equal(st[0], torch.full((D,), float(n), dtype=torch.float64))
    e1, e2 = (st[1] - ref1).abs(), (st[2] - ref2).abs()
    b1, b2 = 1.01 * (chain + 1) * U * abs1, 1.01 * (chain + 3) * U * ref2
    print("R %d D %d offset %g chain %d: sum1 err/bound %.3f  sum2 err/bound %.3f" % (R, D, offset, chain, (e1 / b1).max(), (e2 / b2).max()))
    assert (e1 <= b1).all() and (e2 <= b2).all()
    m1 = st[1] / n
    var = st[2] / n - m1 * m1
    var_ref = ref2 / n - (ref1 / n) ** 2
    bv = 1.01 * U * ((chain + 3) * ref2 / n + 2 * (ref1 / n).abs() * (chain + 1) * abs1 / n)
    print("   var rel err max %.3e (bound %.3e)" % (((var - var_ref).abs() / var_ref).max(), (bv / var_ref).max()))
    assert ((var - var_ref).abs() <= bv).all()
    assert ((s.double().cpu() + m1 - y.double().cpu().view(R, D, 4).mean((0, 2))).abs() <= 1.01 * (chain + 1) * U * abs1 / n + U * offset).all()


# ---------------------------------------------------------------------------------------------- the two necks against float64
def _modules(D, seed):
    """fpn1 / fpn2 as EvBEiT builds them: trunc-normal weights (std 0.02), |bias| <= 0.02, an affine batch norm off its
    initial values.  The transposed convolutions' weights are bf16 values (the rounding the fused path shares with the
    reference)."""
    torch.manual_seed(seed)
    fpn1 = nn.Sequential(nn.ConvTranspose2d(D, D, 2, 2), nn.SyncBatchNorm(D), nn.GELU(), nn.ConvTranspose2d(D, D, 2, 2))
    fpn2 = nn.Sequential(nn.ConvTranspose2d(D, D, 2, 2))
    with torch.no_grad():
        for c in (fpn1[0], fpn1[3], fpn2[0]):
            nn.init.trunc_normal_(c.weight, std=0.02)
            c.weight.copy_(c.weight.to(torch.bfloat16).float())
            c.bias.uniform_(-0.02, 0.02)
        fpn1[1].weight.uniform_(0.8, 1.2)
        fpn1[1].bias.uniform_(-0.2, 0.2)
    return fpn1.cuda().train(), fpn2.cuda().train()


def _inputs(B, D, Hp, Wp, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, D, Hp, Wp), generator=g).to(torch.bfloat16).float()       # zero-mean map, bf16 values
    r1 = torch.randn((B, D, 4 * Hp, 4 * Wp), generator=g)
    r2 = torch.randn((B, D, 2 * Hp, 2 * Wp), generator=g)
    return x, r1, r2


def _ref64(fpn1, fpn2, x, r1=None, r2=None, training=True):
    """fpn1(x), fpn2(x) in float64 on the CPU from the modules' parameters (and, with r1 / r2, the gradients of
    <fpn1(x), r1> + <fpn2(x), r2> w.r.t. x (per neck) and every parameter)."""
    p = {k: v.detach().double().cpu().requires_grad_(True) for k, v in list(fpn1.named_parameters(prefix="fpn1")) +
         list(fpn2.named_parameters(prefix="fpn2"))}
    bn = fpn1[1]
    xa, xb = x.double().clone().requires_grad_(True), x.double().clone().requires_grad_(True)
    y1 = F.conv_transpose2d(xa, p["fpn1.0.weight"], p["fpn1.0.bias"], stride=2)
    if training:
        h = F.batch_norm(y1, None, None, p["fpn1.1.weight"], p["fpn1.1.bias"], True, 0.1, bn.eps)
    else:
        h = F.batch_norm(y1, bn.running_mean.double().cpu(), bn.running_var.double().cpu(), p["fpn1.1.weight"], p["fpn1.1.bias"],
                         False, 0.1, bn.eps)
    o1 = F.conv_transpose2d(F.gelu(h), p["fpn1.3.weight"], p["fpn1.3.bias"], stride=2)
    o2 = F.conv_transpose2d(xb, p["fpn2.0.weight"], p["fpn2.0.bias"], stride=2)
    grads = None
    if r1 is not None:
        ((o1 * r1.double()).sum() + (o2 * r2.double()).sum()).backward()
        grads = dict({k: v.grad for k, v in p.items()}, x1=xa.grad, x2=xb.grad)
    return o1.detach(), o2.detach(), grads


def _rel(a, b):
    return ((a.double().cpu() - b.double()).norm() / b.double().norm()).item()


def _zero_grads(*mods):
    for m in mods:
        for q in m.parameters():
            q.grad = None


def _compare_grads(got, want, names):
    """The bars of tests/test_dense_gpu.py::_compare_grads for bf16 operands: per tensor relative L2 <= 4e-2, pooled cosine
    >= 0.999."""
    fg, fr = [], []
    for k in names:
        rel = _rel(got[k], want[k])
        print("  grad %-16s rel %.3e" % (k, rel))
        assert rel <= 4e-2, (k, rel)
        fg.append(got[k].flatten().double().cpu())
        fr.append(want[k].flatten().double())
    cos = F.cosine_similarity(torch.cat(fg), torch.cat(fr), dim=0).item()
    print("  flat cosine %.6f" % cos)
    assert cos >= 0.999, cos


GRAD_NAMES = ["x1", "x2", "fpn1.0.weight", "fpn1.1.weight", "fpn1.1.bias", "fpn1.3.weight", "fpn1.3.bias", "fpn2.0.weight",
              "fpn2.0.bias"]      # fpn1.0.bias: see test_forward_and_backward_against_float64


@pytest.mark.parametrize("B,D,Hp,Wp", SHAPES)
def test_forward_and_backward_against_float64(B, D, Hp, Wp):
    """fpn2 and fpn1 (train(): batch statistics) against float64 on the CPU, fed the bf16-rounded map and weights.  Behind
    those shared roundings the fused path rounds fpn2 once (the product's output) and fpn1 three times (first product, GELU
    output, second product), each by at most 2^-9 relative: relative L2 per map <= s 2^-8, s = 1 or 3.  The torch modules
    under bf16 autocast on the GPU are measured beside it (printed; no bar of their own).
    Gradients of <fpn1(x), r1> + <fpn2(x), r2>: the input map's (per neck) and the seven parameters' with a non-zero
    gradient against float64 autograd on the same operands.  The eighth, fpn1.0.bias, has the exact gradient 0 (the batch
    norm removes a per-channel constant); the fused path sums the bf16-rounded dY1, whose rounding errors are at most
    2^-9 |dY1| each: |dbias| <= 2^-8 sum |dY1| per channel (a factor 2 for the rounded operands behind dY1)."""
    from mem_amd.necks import FusedNecks
    fpn1, fpn2 = _modules(D, seed=D + Hp)
    x, r1, r2 = _inputs(B, D, Hp, Wp, seed=B * 100 + Wp)
    want1, want2, wg = _ref64(fpn1, fpn2, x, r1, r2)
    nk = FusedNecks(fpn1, fpn2)
    xa, xb = x.cuda().requires_grad_(True), x.cuda().requires_grad_(True)
    o1, o2 = nk.fpn1_apply(xa), nk.fpn2_apply(xb)
    assert o1.dtype == torch.float32 and tuple(o1.shape) == (B, D, 4 * Hp, 4 * Wp) and tuple(o2.shape) == (B, D, 2 * Hp, 2 * Wp)
    e1, e2 = _rel(o1, want1), _rel(o2, want2)
    a1 = a2 = float("nan")
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            a1, a2 = _rel(fpn1(x.cuda()).float(), want1), _rel(fpn2(x.cuda()).float(), want2)
    except RuntimeError as e:                                                       # MIOpen does not take the shape
        print("autocast arm not available:", str(e).splitlines()[0])
    print("shape %s: fpn1 fused %.3e autocast %.3e (bar %.3e) | fpn2 fused %.3e autocast %.3e (bar %.3e)"
          % ((B, D, Hp, Wp), e1, a1, 3 * FWD_BAR, e2, a2, FWD_BAR))
    ((o1 * r1.cuda()).sum() + (o2 * r2.cuda()).sum()).backward()
    got = dict({k: v.grad for k, v in list(fpn1.named_parameters(prefix="fpn1")) + list(fpn2.named_parameters(prefix="fpn2"))},
               x1=xa.grad, x2=xb.grad)
    _compare_grads(got, wg, GRAD_NAMES)
    dY1 = nk._buf("f1.dy1", (B * Hp * Wp, 4 * D)).double().abs().sum(0).view(D, 4).sum(1)
    db = got["fpn1.0.bias"].double().abs()
    print("  fpn1.0.bias: max |grad| / (2^-8 sum |dY1|) = %.3f (float64 autograd: max |grad| %.1e)"
          % ((db / (FWD_BAR * dY1)).max(), wg["fpn1.0.bias"].abs().max()))
    assert (db <= FWD_BAR * dY1).all()
    assert e2 <= FWD_BAR and e1 <= 3 * FWD_BAR, (e1, e2)


def test_batch_norm_bookkeeping_and_eval():
    """After two training calls running_mean, running_var (momentum 0.1, unbiased variance) and num_batches_tracked equal
    nn.BatchNorm2d's on the same data -- the bf16 output of the first transposed convolution, which the two share -- within
    1e-5 relative (vector L2).  eval() normalises with them, changes none of them and keeps nothing for a backward."""
    from mem_amd import necks as N
    B, D, Hp, Wp = 3, 128, 4, 6
    fpn1, fpn2 = _modules(D, seed=3)
    nk = N.FusedNecks(fpn1, fpn2)
    ref = nn.BatchNorm2d(D).double().train()
    for seed in (1, 2):
        x, _, _ = _inputs(B, D, Hp, Wp, seed)
        nk.fpn1_apply(x.cuda().requires_grad_(True))
        y1 = nk._buf("f1.y1", (B * Hp * Wp, 4 * D)).double().cpu()
        ref(N.rows_to_map(y1, B, D, Hp, Wp, 1))
    bn = fpn1[1]
    rm, rv = _rel(bn.running_mean, ref.running_mean), _rel(bn.running_var, ref.running_var)
    print("running_mean rel %.3e running_var rel %.3e" % (rm, rv))
    assert rm <= 1e-5 and rv <= 1e-5
    assert int(bn.num_batches_tracked) == 2 == int(ref.num_batches_tracked)
    fpn1.eval()
    before = (bn.running_mean.clone(), bn.running_var.clone())
    x, _, _ = _inputs(B, D, Hp, Wp, 5)
    out = nk.fpn1_apply(x.cuda().requires_grad_(True))
    assert out.grad_fn is None and not out.requires_grad                          # the forward-only form
    assert nk._fpn1_forward(x.cuda(), keep=False)[1] is None                      # nothing is kept for a backward
    assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1]) and int(bn.num_batches_tracked) == 2
    want1, _, _ = _ref64(fpn1, fpn2, x, training=False)
    e1 = _rel(out, want1)
    print("eval(): fpn1 fused %.3e (bar %.3e)" % (e1, 3 * FWD_BAR))
    assert e1 <= 3 * FWD_BAR
    fpn1.train()
    with torch.no_grad():                                                          # no_grad in train(): batch statistics, forward-only
        out = nk.fpn1_apply(x.cuda())
    assert out.grad_fn is None and int(bn.num_batches_tracked) == 3


def test_syncbn_algebra_through_the_reduce_function():
    """Two half batches, run one after the other as two ranks would, with the reduce function replaced by one that returns
    the sum of both halves' vectors (recorded in a pass before): the forward and every gradient equal the full-batch call
    within the bars above -- and differ from two independent half-batch calls (the second half has 1.5 x the scale, so
    the halves' own statistics are not the batch's)."""
    from mem_amd.necks import FusedNecks
    B, D, Hp, Wp = 4, 128, 4, 6
    fpn1, fpn2 = _modules(D, seed=11)
    x, r1, _ = _inputs(B, D, Hp, Wp, seed=13)
    x[B // 2:] *= 1.5
    names = ["fpn1.0.weight", "fpn1.1.weight", "fpn1.1.bias", "fpn1.3.weight", "fpn1.3.bias"]

    def run(nk, xs, rs):
        xs = xs.cuda().requires_grad_(True)
        out = nk.fpn1_apply(xs)
        (out * rs.cuda()).sum().backward()
        return out.detach().clone(), xs.grad.clone()

    def param_grads():
        g = {k: v.grad.clone() for k, v in fpn1.named_parameters(prefix="fpn1")}
        _zero_grads(fpn1)
        return g

    full = FusedNecks(fpn1, fpn2)
    out_full, dx_full = run(full, x, r1)
    g_full = param_grads()

    halves = [(FusedNecks(fpn1, fpn2), x[:B // 2], r1[:B // 2]), (FusedNecks(fpn1, fpn2), x[B // 2:], r1[B // 2:])]
    store, total = {}, {}

    def reducer(rank):
        def reduce(vec, tag):
            store[(rank, tag)] = vec.clone()
            return total[tag].clone() if tag in total else vec
        return reduce

    for rank, (nk, _, _) in enumerate(halves):
        nk.reduce = reducer(rank)
    results = []
    for tag in (None, "stats", "bwd"):             # pass 0: independent halves; 1: shared statistics; 2: and shared backward sums
        if tag is not None:
            total[tag] = store[(0, tag)] + store[(1, tag)]
        outs = [run(nk, xs, rs) for nk, xs, rs in halves]
        results.append((torch.cat([o for o, _ in outs]), torch.cat([d for _, d in outs]), param_grads()))
    out_ind, dx_ind, _ = results[0]
    out_sync, dx_sync, g_sync = results[2]
    e = _rel(out_sync, out_full.double().cpu())
    print("synchronised halves vs full batch: forward rel %.3e; independent halves: %.3e" % (e, _rel(out_ind, out_full.double().cpu())))
    assert e <= 3 * FWD_BAR
    _compare_grads(dict(g_sync, x1=dx_sync), dict({k: v.double().cpu() for k, v in g_full.items()}, x1=dx_full.double().cpu()),
                   ["x1"] + names)
    assert _rel(out_ind, out_full.double().cpu()) > 5 * 3 * FWD_BAR
    assert _rel(dx_ind, dx_full.double().cpu()) > 4e-2


# ---------------------------------------------------------------------------------------------- EvBEiT end to end
CFG = dict(img_size=(64, 96), patch_size=16, in_chans=3, embed_dim=128, depth=4, num_heads=2, out_indices=(0, 1, 2, 3),
           use_rel_pos_bias=True, use_abs_pos_emb=False, init_values=0.1, drop_path_rate=0.0)


def _evbeit(sd=None, **kw):
    from mem_amd.semseg_backbone import EvBEiT
    from oracle.vit_ref import fill_by_name
    m = EvBEiT(**CFG, **kw)
    if sd is None:
        trunk = {k: v for k, v in m.state_dict().items() if not k.startswith("fpn")}
        m.load_state_dict(fill_by_name(trunk, seed=5), strict=False)
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        for k in ("fpn1.0.weight", "fpn1.3.weight", "fpn2.0.weight"):             # bf16 values: a rounding both modes share
            sd[k] = sd[k].to(torch.bfloat16).float()
    m.load_state_dict(sd)
    return m.cuda(), sd


def _x(B=4, seed=3):
    from oracle.gen_golden_ft import ft_inputs
    return ft_inputs(dict(in_chans=3, img_size=(64, 96), num_classes=2), B, seed)[0].cuda()


def test_evbeit_fused_against_torch_necks():
    """The same weights under necks="torch" and necks="fused": fpn3 / fpn4 outputs bit-identical, fpn1 / fpn2 within the
    forward bar (the torch arm is fp32 on the unrounded map: the map's bf16 rounding, 2^-9 relative at most and 2^-9 / sqrt 3
    rms, is one more of the roundings the bar counts double), in train() (batch statistics, drop path 0) and eval(); and
    necks="torch" is bit-identical to a model built without the argument.
    The bit comparison of the two torch arms runs under torch.backends.cudnn.flags(deterministic=True): MIOpen's default
    choice for nn.ConvTranspose2d in fp32 is not reproducible from call to call (measured on MI355X, one module, one input,
    two calls: max difference 2.4e-7 at D = 128; bit-identical with the flag), so without it the torch path differs from
    itself."""
    m0, sd = _evbeit()
    mt, _ = _evbeit(sd, necks="torch")
    mf, _ = _evbeit(sd, necks="fused")
    x = _x()
    for mode in ("train", "eval"):
        for m in (m0, mt, mf):
            getattr(m, mode)()
        with torch.no_grad(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
            o0 = [o.clone() for o in m0(x)]
            ot = [o.clone() for o in mt(x)]
            of = [o.clone() for o in mf(x)]
        print("%s: default == necks=\"torch\" per level: %s" % (mode, [torch.equal(a, b) for a, b in zip(o0, ot)]))
        assert all(torch.equal(a, b) for a, b in zip(o0, ot)), mode
        assert [tuple(o.shape) for o in of] == [tuple(o.shape) for o in ot]
        assert torch.equal(of[2], ot[2]) and torch.equal(of[3], ot[3])
        e1, e2 = _rel(of[0], ot[0].double().cpu()), _rel(of[1], ot[1].double().cpu())
        print("%s: fpn1 fused vs torch fp32 %.3e (bar %.3e), fpn2 %.3e (bar %.3e)" % (mode, e1, 3 * FWD_BAR, e2, FWD_BAR))
        assert e1 <= 3 * FWD_BAR and e2 <= FWD_BAR
    assert int(mf.fpn1[1].num_batches_tracked) == 1 == int(mt.fpn1[1].num_batches_tracked)


def test_evbeit_fused_training_step_and_single_level_gradients():
    """One FlatAdamW step through necks="fused" moves every neck parameter and the trunk; a training call with gradient at
    one pyramid level only leaves the other neck's gradients exactly zero."""
    from mem_amd import optim_factory as OF
    m, _ = _evbeit(necks="fused")
    m.train()
    with contextlib.redirect_stdout(io.StringIO()):
        groups = OF.get_parameter_groups(m, 0.05, m.no_weight_decay())
    opt = OF.FlatAdamW(m, groups, lr=1e-3)
    x = _x()
    neck = [k for k, _ in m.named_parameters() if k.startswith("fpn")]
    assert len(neck) == 8
    for level, mine in ((0, "fpn1."), (1, "fpn2.")):
        outs = m(x)
        outs[level].square().mean().backward()
        for k, p in m.named_parameters():
            if k in neck and not k.startswith(mine):
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, (level, k)
        for k in neck:
            if k.startswith(mine) and k != "fpn1.0.bias":                          # (its exact gradient is 0)
                assert float(dict(m.named_parameters())[k].grad.abs().max()) > 0.0, (level, k)
        assert float(m.blocks[0].attn.qkv.weight.grad.abs().max()) > 0.0
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    outs = m(x)
    assert all(o.requires_grad for o in outs[:3])
    sum(o.float().square().mean() for o in outs).backward()
    opt.step()
    torch.cuda.synchronize()
    moved = {k: not torch.equal(p.detach(), before[k]) for k, p in m.named_parameters()}
    assert all(torch.isfinite(p).all() for p in m.parameters())
    for k in neck + ["patch_embed.proj.weight", "cls_token", "blocks.0.attn.qkv.weight", "blocks.3.mlp.fc2.weight", "blocks.3.gamma_2",
                     "blocks.1.attn.relative_position_bias_table"]:
        assert moved[k], k
    v0 = m._fused_necks._stamp
    with torch.no_grad():
        outs = m(x)                                                                # the step's weights: the transposed copies are re-made once
    assert m._fused_necks._stamp != v0 and all(torch.isfinite(o).all() for o in outs)
    v1 = m._fused_necks._stamp
    with torch.no_grad():
        m(x)
    assert m._fused_necks._stamp == v1                                             # and not per forward
