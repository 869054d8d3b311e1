"""-m gpu: the kernels every training step ends in -- grad norm, AdamW (plain and per-group), the bf16 shadow-weight movers
(cast, transpose_cast, transpose_cast_batched), transpose_bf16 with its fused column sums, and the zero fill -- element by
element against float64 (step_tail_ref.py) or bit for bit against torch's round-to-nearest-even bf16.

Bars follow from the fp32 arithmetic (step_tail_ref's running bound), never from what the kernels give; the measured figure
is printed next to every bar.  Regions a kernel must not write hold a NaN bit pattern and are compared bit for bit.

Measured on an MI355X, worst |err| / bound over every case of this file (bar 2): p 0.499, m 0.991, v 0.985; the norm
0.223 of its 2u (bar 2).  None is near the bar: both kernels divide and take the square root correctly rounded and
contract to FMA, which only removes roundings.  adamw_kernel and adamw_groups_kernel compile to the same arithmetic
(same opcode mix in their gfx950 assembly), and the two-row-table test finds them bit-identical.  The whole file runs in
about 4 s."""
import numpy as np
import pytest
import torch

import step_tail_ref as R

pytestmark = pytest.mark.gpu

NAN32, NAN16, NAN64 = 0x7FC0BEEF, 0x7FC1, 0x7FF8DEADBEEF0001
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64, torch.uint8: torch.uint8}
DEV = "cuda"


def _bits(t):
    return t.view(_INT[t.dtype])


def _canvas(shape, dtype):
    """a device buffer filled with the NaN canary"""
    t = torch.empty(shape, dtype=dtype, device=DEV)
    if dtype == torch.uint8:
        t.fill_(0xA5)
    else:
        _bits(t).fill_({torch.float32: NAN32, torch.bfloat16: NAN16, torch.float64: NAN64}[dtype])
    return t


def _same_bits(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


def _call(fn, *args):
    from mem_amd import _lib
    _lib.check(fn(*args, _lib.stream_ptr()), fn.__name__)


def _lib():
    from mem_amd import _lib, ops  # noqa: F401  (ops declares the signatures)
    return _lib.lib


# ================================================================================================ grad_norm
def _norm_values(n, seed):
    """fp32 values spanning 2^-20 .. 2^10: a mantissa in [1, 2) times a random power of two, random sign"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    mant = 1.0 + torch.rand(n, generator=g, device=DEV, dtype=torch.float64)
    e = torch.randint(-20, 10, (n,), generator=g, device=DEV)
    sign = torch.randint(0, 2, (n,), generator=g, device=DEV).double() * 2 - 1
    return (torch.ldexp(mant, e) * sign).float()


@pytest.mark.parametrize("n", [0, 4, 1020, 1024 * 37, 4 * (2 * 262144 + 77)])
def test_grad_norm_against_float64(n):
    """sqrt(sum x^2): the pair x^2 + y^2 in fp32 is within 2u of the exact pair, the rest of the sum is float64, so the
    norm is within u before the final cast and 2u after it.  Bar: twice that."""
    from mem_amd import ops
    x = _norm_values(max(n, 4), 50 + n % 97)[:max(n, 4)]
    nb = min(1024, max(1, (n // 4 + 255) // 256))
    ws = _canvas((1024 + 16,), torch.float64)
    ws0 = ws.clone()
    out = _canvas((4,), torch.float32)
    ops.grad_norm(x, n, out, ws[:1024])
    ref = float(x[:n].double().norm().item())
    got = float(out[0].item())
    fig = abs(got - ref) / (2 * R.U * ref) if ref > 0 else (0.0 if got == 0.0 else float("inf"))
    print("\n  grad_norm n=%d  blocks=%d  |err| / (2u norm) = %.3f (bar 2)" % (n, nb, fig))
    assert fig <= 2.0, (n, got, ref)
    assert _same_bits(out[1:], _canvas((3,), torch.float32))
    assert _same_bits(ws[nb:], ws0[nb:]), "workspace beyond the partial sums was written"
    assert not _same_bits(ws[:nb], ws0[:nb])
    out2 = _canvas((4,), torch.float32)
    ops.grad_norm(x, n, out2, ws[:1024])
    assert _same_bits(out, out2), "two calls differ"


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_grad_norm_propagates_non_finite(bad):
    from mem_amd import ops
    n = 1024 * 37
    x = _norm_values(n, 61)
    x[n - 3] = bad
    ws, out = torch.zeros(1024, dtype=torch.float64, device=DEV), torch.zeros(1, device=DEV)
    ops.grad_norm(x, n, out, ws)
    got = float(out.item())
    assert (got != got) if bad != bad else got == float("inf"), got


# ================================================================================================ adamw
H = R.HYPER
NA = 1024 * 37


def _run_adamw(p, g, m, v, flags, step, gnorm, max_norm, wd=None, n=None):
    from mem_amd import ops
    ops.adamw(p, g, m, v, p.numel() if n is None else n, flags, H["lr"], H["b1"], H["b2"], H["eps"], H["wd"] if wd is None else wd,
              step, gnorm=gnorm, max_norm=max_norm)


def _device_norm(g32):
    from mem_amd import ops
    ws, out = torch.zeros(1024, dtype=torch.float64, device=DEV), torch.zeros(1, device=DEV)
    ops.grad_norm(g32, g32.numel(), out, ws)
    return out


def _check64(got, ref, err, what, worst):
    figs = []
    for k, gk, rk, ek in zip("pmv", got, ref, err):
        f = R.worst_ratio(gk, rk, ek, R.TINY)
        worst[k] = max(worst[k], f)
        figs.append(f)
        assert f <= 2.0, (what, k, f)
    return figs


@pytest.fixture(scope="module")
def adam_states():
    """family -> (g, flags u8, flags per element, {step: state}) on the device, computed once and never modified"""
    out = {}
    for fi, (ps, gs) in enumerate(R.FAMILIES):
        p, g = R.family_inputs(NA, ps, gs, 200 + fi, DEV)
        flags = R.seeded_flags(NA // 1024, 11, DEV)
        fe = flags.bool().repeat_interleave(1024)
        out[fi] = (g, flags, fe, R.teacher_states(p, g, fe, R.STEPS))
    return out


CLIP = ("off_no_gnorm", "off_finite_gnorm", "clamped_to_1", "clipped")


@pytest.mark.parametrize("clip", CLIP)
@pytest.mark.parametrize("fi", range(len(R.FAMILIES)))
def test_adamw_against_float64(adam_states, fi, clip):
    """p, m and v of one kernel step from the reference's fp32 state, steps 1, 2, 3, 50, 1000: within 2 x the running
    bound + 2^-149 of float64."""
    g, flags, fe, st = adam_states[fi]
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for step in R.STEPS:
        p0, m0, v0 = st[step]
        gt = R.grad_at(g, step)
        g32 = gt.float()
        gn = _device_norm(g32)
        gnf = float(gn.item())
        max_norm, gnorm = {"off_no_gnorm": (0.0, None), "off_finite_gnorm": (0.0, gn), "clamped_to_1": (2.0 * gnf, gn),
                           "clipped": (0.37 * gnf, gn)}[clip]
        max_norm = R.f32(max_norm)
        coef, on = R.coef_ref(gnf, max_norm)
        assert (coef == 1.0) == (clip != "clipped") and on == (max_norm > 0)
        sc = dict(R.host_scalars(step=step, **H), coef=coef)
        decay = torch.where(fe, torch.full_like(p0, sc["decay"]), torch.ones_like(p0))
        ref, err = R.adamw_ref(p0, gt, m0, v0, sc, decay, sc["step_size"], on)
        p, m, v = p0.float(), m0.float(), v0.float()
        _run_adamw(p, g32, m, v, flags, step, gnorm, max_norm)
        assert torch.equal(g32.double(), gt), "the gradient was written"
        _check64((p, m, v), ref, err, (R.FAMILIES[fi], clip, step), worst)
        assert not torch.equal(m.double(), m0) and not torch.equal(v.double(), v0)
    print("\n  adamw |p|%g |g|%g %-16s worst |err| / bound: p %.3f  m %.3f  v %.3f (bar 2)" % (*R.FAMILIES[fi], clip, worst["p"], worst["m"], worst["v"]))


def test_adamw_without_weight_decay(adam_states):
    """wd = 0: decay_mul == 1 whatever the flags say"""
    g, flags, fe, st = adam_states[0]
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for step in (1, 50):
        p0, m0, v0 = st[step]
        gt = R.grad_at(g, step)
        sc = R.host_scalars(H["lr"], H["b1"], H["b2"], H["eps"], 0.0, step)
        assert sc["decay"] == 1.0
        ref, err = R.adamw_ref(p0, gt, m0, v0, sc, 1.0, sc["step_size"], False)
        p, m, v = p0.float(), m0.float(), v0.float()
        _run_adamw(p, gt.float(), m, v, flags, step, None, 0.0, wd=0.0)
        _check64((p, m, v), ref, err, ("wd=0", step), worst)
    print("\n  adamw wd=0 worst |err| / bound: p %.3f  m %.3f  v %.3f (bar 2)" % (worst["p"], worst["m"], worst["v"]))


def test_adamw_second_loop_trip():
    """2 * 8192 + 5 chunks: every workgroup walks two chunks, five walk three.  The whole-buffer call equals three uneven
    calls on chunk-aligned slices bit for bit (the pipelined optimizer's calls), and 64 chunks -- the first and last of every
    trip and 58 seeded others -- are checked against float64.  Flags of chunks c and c +- 8192 differ."""
    nch = 2 * 8192 + 5
    n = nch * 1024
    gen = torch.Generator(device=DEV).manual_seed(77)
    p0 = (torch.randn(n, generator=gen, device=DEV) * 0.02)
    g = (torch.randn(n, generator=gen, device=DEV) * 1e-3)
    m0 = (torch.randn(n, generator=gen, device=DEV) * 1e-3)
    v0 = (torch.rand(n, generator=gen, device=DEV) * 1e-6)
    c = torch.arange(nch, device=DEV)
    flags = (R.seeded_flags(8192, 13, DEV)[c % 8192] ^ ((c // 8192) & 1).to(torch.uint8)).contiguous()
    assert bool((flags[:8192] != flags[8192:16384]).all()) and bool((flags[16384:] != flags[8192:8197]).all())
    step = 3
    gn = _device_norm(g)
    max_norm = R.f32(0.5 * float(gn.item()))
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    _run_adamw(p, g, m, v, flags, step, gn, max_norm)
    ps, ms, vs = p0.clone(), m0.clone(), v0.clone()
    cuts = (0, 5000, 13001, nch)
    for c0, c1 in zip(cuts[:-1], cuts[1:]):
        a, b = c0 * 1024, c1 * 1024
        _run_adamw(ps[a:b], g[a:b], ms[a:b], vs[a:b], flags[c0:c1], step, gn, max_norm)
    assert _same_bits(p, ps) and _same_bits(m, ms) and _same_bits(v, vs), "sliced calls differ from the whole-buffer call"
    pick = torch.tensor([0, 8191, 8192, 16383, 16384, 16388], device=DEV)
    rest = torch.randperm(nch, generator=gen, device=DEV)
    rest = rest[~torch.isin(rest, pick)][:58]
    pick = torch.cat([pick, rest])
    idx = (pick[:, None] * 1024 + torch.arange(1024, device=DEV)[None, :]).flatten()
    coef, on = R.coef_ref(float(gn.item()), max_norm)
    sc = dict(R.host_scalars(step=step, **H), coef=coef)
    fe = flags[pick].bool().repeat_interleave(1024)
    assert on and coef < 1 and bool(fe.any()) and not bool(fe.all())
    q = [t[idx].double() for t in (p0, g, m0, v0)]
    decay = torch.where(fe, torch.full_like(q[0], sc["decay"]), torch.ones_like(q[0]))
    ref, err = R.adamw_ref(*q, sc, decay, sc["step_size"], True)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    _check64((p[idx], m[idx], v[idx]), ref, err, "second trip", worst)
    print("\n  adamw %d chunks, 64 checked: worst |err| / bound: p %.3f  m %.3f  v %.3f (bar 2)" % (nch, worst["p"], worst["m"], worst["v"]))


# ================================================================================================ adamw_groups
NG = 1024 * 40


def _group_setup(step):
    """256 groups (layer-wise lr decay x {decay, no decay}); group 7 is frozen {1, 0}; ids 0 and 255 are in use"""
    bc1 = 1.0 - H["b1"] ** step
    table = np.zeros((256, 2), dtype=np.float32)
    for k in range(256):
        lr_g = H["lr"] * 0.97 ** (k // 2)
        wd_g = H["wd"] if k % 2 == 0 else 0.0
        table[k] = (np.float32(1.0 - lr_g * wd_g), np.float32(lr_g / bc1))         # host double, rounded once
    table[7] = (1.0, 0.0)
    gen = torch.Generator(device="cpu").manual_seed(21)
    ids = torch.randint(0, 256, (NG // 1024,), generator=gen, dtype=torch.uint8)
    ids[ids == 7] = 8
    ids[0], ids[1], ids[2], ids[-1] = 0, 255, 7, 7
    return torch.from_numpy(table).to(DEV), ids.to(DEV)


def _run_groups(p, g, m, v, ids, table, n_groups, step, gnorm, max_norm):
    from mem_amd import ops
    ops.adamw_groups(p, g, m, v, p.numel(), ids, table, n_groups, H["b1"], H["b2"], H["eps"], step, gnorm=gnorm, max_norm=max_norm)


@pytest.mark.parametrize("clipped", [False, True])
def test_adamw_groups_against_float64(clipped):
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for fi, (ps, gs) in enumerate(R.FAMILIES):
        p0, g = R.family_inputs(NG, ps, gs, 300 + fi, DEV)
        st = R.teacher_states(p0, g, torch.ones(NG, dtype=torch.bool, device=DEV), (1, 3, 50))
        for step in (1, 3, 50):
            table, ids = _group_setup(step)
            p0, m0, v0 = st[step]
            gt = R.grad_at(g, step)
            g32 = gt.float()
            gn = _device_norm(g32)
            max_norm = R.f32(0.37 * float(gn.item())) if clipped else 0.0
            coef, on = R.coef_ref(float(gn.item()), max_norm)
            sc = dict(R.host_scalars(step=step, **H), coef=coef)
            per = table[ids.long()].double().repeat_interleave(1024, 0)
            ref, err = R.adamw_ref(p0, gt, m0, v0, sc, per[:, 0].contiguous(), per[:, 1].contiguous(), on)
            p, m, v = p0.float(), m0.float(), v0.float()
            _run_groups(p, g32, m, v, ids, table, 256, step, gn if clipped else None, max_norm)
            _check64((p, m, v), ref, err, ("groups", R.FAMILIES[fi], step), worst)
            frozen = (ids == 7).repeat_interleave(1024)
            assert int(frozen.sum()) == 2048
            assert _same_bits(p[frozen], p0.float()[frozen]), "a frozen group's parameters moved"
            assert bool((m[frozen] != m0.float()[frozen]).any()) and bool((v[frozen] != v0.float()[frozen]).any())
            assert not _same_bits(p[~frozen], p0.float()[~frozen])
    print("\n  adamw_groups clipped=%s worst |err| / bound: p %.3f  m %.3f  v %.3f (bar 2)" % (clipped, worst["p"], worst["m"], worst["v"]))


@pytest.mark.parametrize("clipped", [False, True])
def test_adamw_groups_two_rows_equal_adamw_bit_for_bit(adam_states, clipped):
    """group table {1, step_size}, {decay_mul, step_size} indexed by the flags == adamw"""
    g, flags, fe, st = adam_states[0]
    for step in (1, 50):
        p0, m0, v0 = st[step]
        g32 = R.grad_at(g, step).float()
        gn = _device_norm(g32)
        max_norm = R.f32(0.37 * float(gn.item())) if clipped else 0.0
        sc = R.host_scalars(step=step, **H)
        table = torch.tensor([[1.0, sc["step_size"]], [sc["decay"], sc["step_size"]]], dtype=torch.float32, device=DEV)
        a = [t.float() for t in (p0, m0, v0)]
        b = [t.float() for t in (p0, m0, v0)]
        _run_adamw(a[0], g32, a[1], a[2], flags, step, gn if clipped else None, max_norm)
        _run_groups(b[0], g32, b[1], b[2], flags, table, 2, step, gn if clipped else None, max_norm)
        for k, x, y in zip("pmv", a, b):
            assert _same_bits(x, y), (k, step, int((_bits(x) != _bits(y)).sum()))


# ================================================================================================ non-finite guard
@pytest.mark.parametrize("kernel", ["adamw", "adamw_groups"])
@pytest.mark.parametrize("max_norm", [0.0, 1.0])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_norm_skips_the_update(kernel, max_norm, bad):
    n = 1024 * 3
    p0, g = R.family_inputs(n, 0.02, 1e-3, 400, DEV)
    gen = torch.Generator(device=DEV).manual_seed(5)
    p0, g = p0.float(), g.float()
    m0, v0 = torch.randn(n, generator=gen, device=DEV) * 1e-3, torch.rand(n, generator=gen, device=DEV) * 1e-6
    flags = torch.tensor([1, 0, 1], dtype=torch.uint8, device=DEV)
    sc = R.host_scalars(step=2, **H)
    table = torch.tensor([[1.0, sc["step_size"]], [sc["decay"], sc["step_size"]]], dtype=torch.float32, device=DEV)

    def run(p, m, v, gn):
        if kernel == "adamw":
            _run_adamw(p, g, m, v, flags, 2, gn, max_norm)
        else:
            _run_groups(p, g, m, v, flags, table, 2, 2, gn, max_norm)

    p, m, v = p0.clone(), m0.clone(), v0.clone()
    run(p, m, v, torch.tensor([bad], device=DEV))
    assert _same_bits(p, p0) and _same_bits(m, m0) and _same_bits(v, v0), "a non-finite norm let the update through"
    run(p, m, v, torch.tensor([0.5], device=DEV))
    for x, x0 in ((p, p0), (m, m0), (v, v0)):
        assert bool(torch.isfinite(x).all()) and float((x != x0).float().mean()) > 0.9


# ================================================================================================ cast
def _cast(src, n, pad=16):
    from mem_amd import ops
    dst = _canvas((n + pad,), torch.bfloat16)
    ops.cast_f32_bf16(src, dst, n)
    assert _same_bits(dst[n:], _canvas((pad,), torch.bfloat16)), "cast wrote beyond n"
    return dst[:n]


def test_cast_second_loop_trip_and_offset_source():
    n = 4 * (2 * 4096 * 256 + 3)
    gen = torch.Generator(device=DEV).manual_seed(90)
    buf = torch.randn(n + 4, generator=gen, device=DEV) * torch.exp(torch.randn(n + 4, generator=gen, device=DEV) * 3)
    assert _same_bits(_cast(buf, n), buf[:n].bfloat16())
    src = buf[4:]                                                     # 16 bytes in
    assert src.data_ptr() % 16 == 0
    assert _same_bits(_cast(src, n), src[:n].bfloat16())
    assert _same_bits(_cast(src, 4), src[:4].bfloat16())
    before = _canvas((8,), torch.bfloat16)
    from mem_amd import ops
    ops.cast_f32_bf16(src, before, 0)
    assert _same_bits(before, _canvas((8,), torch.bfloat16))


def test_cast_rounds_to_nearest_even():
    bits = [
        0x3F808000,   # 1 + 2^-8: tie, even below   -> 0x3F80
        0x3F818000,   # tie, even above            -> 0x3F82
        0xBF808000, 0xBF818000,                    # the same, negative
        0x3F808001,   # just above the tie         -> 0x3F81
        0x3F807FFF,   # just below the tie         -> 0x3F80
        0x3FFF8000,   # tie with a mantissa carry into the next exponent -> 0x4000 (2.0)
        0x3FFFFFFF,   # carry                      -> 0x4000
        0x00000000, 0x80000000,                    # +-0
        0x7F800000, 0xFF800000,                    # +-inf
        0x7F7FFFFF, 0xFF7FFFFF,                    # +-FLT_MAX -> +-inf
        0x7F7F7FFF,   # the largest value that stays finite -> 0x7F7F
        0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FBFFFFF,      # NaNs (the last two signalling, payload in the low bits only)
    ]
    want = [0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F81, 0x3F80, 0x4000, 0x4000, 0x0000, 0x8000, 0x7F80, 0xFF80, 0x7F80, 0xFF80, 0x7F7F]
    while len(bits) % 4:
        bits.append(0x3F800000)
    src = torch.tensor(np.array(bits, dtype=np.uint32).view(np.int32), device=DEV).view(torch.float32)
    got = _cast(src, len(bits))
    ref = src.bfloat16()
    nan = torch.isnan(src)
    assert int(nan.sum()) == 4
    assert bool(torch.isnan(got[nan]).all()), "a NaN did not stay a NaN"
    assert _same_bits(got[~nan], ref[~nan])
    w = torch.tensor(np.array(want, dtype=np.uint16).view(np.int16), device=DEV)
    assert torch.equal(_bits(got)[:len(want)], w), (_bits(got)[:len(want)].tolist(), w.tolist())


# ================================================================================================ transposes
# (R, Cc, ldin, ldout, source offset in floats)
T_SHAPES = [(64, 64, 64, 64, 0), (70, 100, 100, 72, 0), (70, 100, 101, 80, 0), (70, 100, 100, 200, 0), (1, 8, 8, 8, 0),
            (130, 65, 68, 136, 0), (192, 48, 48, 192, 0), (70, 100, 100, 72, 1)]
EXTRA_ROWS = 3


def _t_source(R_, Cc, ldin, off, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    buf = torch.randn(R_ * ldin + 8, generator=gen, device=DEV)
    assert buf.data_ptr() % 16 == 0
    src = buf[off:off + R_ * ldin]
    assert (src.data_ptr() % 16 == 0) == (off % 4 == 0)
    return buf, src


def _t_expected(src, R_, Cc, ldin, ldout):
    """the canvas after the call: the bf16 transpose, zeros up to min(ldout, 64-padded R), canary everywhere else"""
    exp = _canvas((Cc + EXTRA_ROWS, ldout), torch.bfloat16)
    rp = min(ldout, (R_ + 63) // 64 * 64)
    exp[:Cc, :rp] = 0
    exp[:Cc, :R_] = src.view(R_, ldin)[:, :Cc].bfloat16().t()
    return exp


@pytest.fixture(scope="module")
def t_cases():
    """per shape: (source buffer, source view, expected canvas), never modified"""
    out = []
    for k, (R_, Cc, ldin, ldout, off) in enumerate(T_SHAPES):
        buf, src = _t_source(R_, Cc, ldin, off, 500 + k)
        out.append((buf, src, _t_expected(src, R_, Cc, ldin, ldout)))
    return out


@pytest.mark.parametrize("k", range(len(T_SHAPES)))
def test_transpose_cast_single(t_cases, k):
    lib = _lib()
    R_, Cc, ldin, ldout, off = T_SHAPES[k]
    _, src, exp = t_cases[k]
    out = _canvas((Cc + EXTRA_ROWS, ldout), torch.bfloat16)
    _call(lib.memhip_transpose_cast_f32_bf16, src.data_ptr(), ldin, R_, Cc, out.data_ptr(), ldout)
    rp = min(ldout, (R_ + 63) // 64 * 64)
    assert _same_bits(out[:Cc, :R_], exp[:Cc, :R_]), "transposed values"
    assert int(_bits(out[:Cc, R_:rp]).abs().sum()) == 0, "zero fill"
    assert _same_bits(out[:Cc, rp:], exp[:Cc, rp:]) and _same_bits(out[Cc:], exp[Cc:]), "written beyond the fill"


def _descs(t_cases, outs, which):
    desc = np.zeros((len(which), 6), dtype=np.int64)
    prefix = np.zeros(len(which) + 1, dtype=np.int32)
    for j, k in enumerate(which):
        R_, Cc, ldin, ldout, _ = T_SHAPES[k]
        desc[j] = (t_cases[k][1].data_ptr(), ldin, R_, Cc, outs[k].data_ptr(), ldout)
        prefix[j + 1] = prefix[j] + ((R_ + 63) // 64) * ((Cc + 63) // 64)
    return desc, prefix


def _fresh_outs():
    outs = [_canvas((Cc + EXTRA_ROWS, ldout), torch.bfloat16) for (_, Cc, _, ldout, _) in T_SHAPES]
    for o in outs:
        assert o.data_ptr() % 16 == 0
    return outs


def test_transpose_cast_batched_all_shapes_in_one_launch(t_cases):
    from mem_amd import ops
    outs = _fresh_outs()
    desc, prefix = _descs(t_cases, outs, range(len(T_SHAPES)))
    d, pf = torch.from_numpy(desc).to(DEV), torch.from_numpy(prefix).to(DEV)
    ops.transpose_cast_batched(d, pf, len(T_SHAPES), int(prefix[-1]))
    for k, o in enumerate(outs):
        assert _same_bits(o, t_cases[k][2]), ("batched != single-call result", T_SHAPES[k])


def test_transpose_cast_batched_slice_and_empty(t_cases):
    """the pipelined optimizer's launches: desc[k0 : k0 + n] with a prefix that restarts at 0 writes those outputs only"""
    from mem_amd import ops
    outs = _fresh_outs()
    desc, prefix = _descs(t_cases, outs, range(len(T_SHAPES)))
    d = torch.from_numpy(desc).to(DEV)
    k0, n = 2, 3
    loc = (prefix[k0:k0 + n + 1] - prefix[k0]).astype(np.int32)
    # local prefixes of several buckets in one array, as the engine keeps them
    allp = torch.from_numpy(np.concatenate([np.array([0, 1], dtype=np.int32), loc, np.array([0, 4], dtype=np.int32)])).to(DEV)
    ops.transpose_cast_batched(d, allp[2:], 0, 7)                       # n == 0
    ops.transpose_cast_batched(d, allp[2:], 3, 0)                       # total_tiles == 0
    for k, (_, Cc, _, ldout, _) in enumerate(T_SHAPES):
        assert _same_bits(outs[k], _canvas((Cc + EXTRA_ROWS, ldout), torch.bfloat16)), "an empty launch wrote"
    ops.transpose_cast_batched(d[k0:k0 + n], allp[2:2 + n + 1], n, int(loc[-1]))
    for k, (_, Cc, _, ldout, _) in enumerate(T_SHAPES):
        want = t_cases[k][2] if k0 <= k < k0 + n else _canvas((Cc + EXTRA_ROWS, ldout), torch.bfloat16)
        assert _same_bits(outs[k], want), ("slice launch", k)


# ------------------------------------------------------------------------------------------------ transpose_bf16 + sums
@pytest.mark.parametrize("R_,Cc,Rp,r0,r1", [
    (394, 2304, 448, (5, 77), (60, 2304)),          # unaligned range; a second one overlapping it
    (394, 2304, 448, (0, 768), None),
    (394, 2304, 448, None, (2300, 2304)),
    (394, 2304, 448, None, None),                   # both sum pointers null
    (5, 100, 64, (5, 77), (70, 100)),
    (0, 72, 64, (5, 70), (0, 72)),                  # no rows: zeros out, sums unchanged
])
def test_transpose_bf16_with_column_sums(R_, Cc, Rp, r0, r1):
    """integer inputs in [-4, 4]: every partial column sum is an integer below 2^24, so the atomics are exact in any order"""
    from mem_amd import ops
    gen = torch.Generator(device=DEV).manual_seed(600 + R_)
    a = torch.randint(-4, 5, (max(R_, 1), Cc), generator=gen, device=DEV).to(torch.bfloat16)
    ldout = Rp + 8
    out = _canvas((Cc + 2, ldout), torch.bfloat16)
    exp = out.clone()
    exp[:Cc, :Rp] = 0
    exp[:Cc, :R_] = a[:R_].t()

    def sums(r):
        if r is None:
            return None, None
        buf = _canvas((r[1] - r[0] + 5,), torch.float32)
        buf[:r[1] - r[0]] = torch.randint(-9, 10, (r[1] - r[0],), generator=gen, device=DEV).float()
        want = buf.clone()
        want[:r[1] - r[0]] += a[:R_, r[0]:r[1]].double().sum(0).float()
        return buf, want

    cs0, w0 = sums(r0)
    cs1, w1 = sums(r1)
    ops.transpose_bf16(a, R_, Cc, out, Rp, cs0, r0 or (0, 0), cs1, r1 or (0, 0))
    assert _same_bits(out, exp), "transposed tile / zero fill / canary"
    for cs, w in ((cs0, w0), (cs1, w1)):
        if cs is not None:
            assert _same_bits(cs, w), ("column sums", float((cs[:-5] - w[:-5]).abs().max()))


# ================================================================================================ zero
@pytest.mark.parametrize("nbytes", [16, 2 * 2048 * 256 * 16 + 48])
def test_zero_fill_and_its_neighbours(nbytes):
    from mem_amd import ops
    buf = _canvas((nbytes + 64,), torch.uint8)
    assert buf.data_ptr() % 16 == 0
    ops.zero_(buf[32:32 + nbytes])
    assert int(buf[32:32 + nbytes].max()) == 0
    assert bool((buf[:32] == 0xA5).all()) and bool((buf[32 + nbytes:] == 0xA5).all()), "zero wrote outside its range"
