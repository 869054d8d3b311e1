"""The tokenizer's convolutions at layer level, EXACTLY, on non-square layers (H != W and Ho != Wo in every case), for each of
the seven kernel forms conv_plan.cpp chooses from (csrc/conv.hip: bf16; csrc/conv_f32.hip: fp32, static and dynamic batch;
csrc/conv_f16x2.hip: two fp16 planes per value, <4> / <8> / wide / first layer), plus the layout and certification plumbing
(nchw_to_padded_nhwc4, tok_gather_images, tok_scatter_ids) and a non-square tokenizer end to end in all three precisions.

Exact checks: the reference is torch.nn.functional.conv2d in float64 on the same values, compared with torch.equal after
conversion to the output format -- no tolerance.  Two kinds of operands:
  tap selector    one-hot weights (+1 / -1 at one (ky, kx, c) per output channel) on a position-coded input: every output is
                  one shifted, strided copy of the input, so a wrong tap, stride, padding offset, H / W swap or channel chunk
                  is a hard mismatch.  The selectors of a few launches cover every (ky, kx) and every element position of a
                  k-tile (all of K where K <= 8 C_out); asserted per layer (_assert_cover).
  small integers  x and w in {-1, 0, 1}, integer bias and residual: catches a dropped or doubled k-tile.
Each case first asserts ON THE REFERENCE ALONE that every expected value (before and after the residual add) is exactly
representable in the output format (_assert_representable), so a mismatch is the kernel's.  These preconditions, and the
selector coverage, were evaluated for every committed shape and seed with the float64 reference on the CPU (they do not
depend on the device: all sums are exact in float64 in any order).
Every output buffer is filled with a NaN canary bit pattern first (the border of a padded output, three rows behind a dense
matrix, the slots behind the live samples of a dynamic batch, a guard behind every plane) and everything outside the written
region must be unchanged bit for bit; the residual's border and, where pad = 0, the input's border hold NaN as well."""
from typing import NamedTuple, Optional

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp16x2": torch.float16}
BK = {"bf16": 64, "fp32": 32, "fp16x2": 64}                      # k-tile of the mode's kernels (elements)
CANARY = {torch.float32: 0x7FC0BEEF, torch.bfloat16: 0x7FC1, torch.float16: 0x7E01}         # NaN bit patterns
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
TILE_M, TILE_N, SMALL_M, WIDE_M = 128, 128, 32, 256


def _device():
    return "cuda" if torch.cuda.is_available() else "cpu"


def _cdiv(a, b):
    return (a + b - 1) // b


class Layer(NamedTuple):
    mode: str
    B: int
    H: int
    W: int
    cin: int
    cout: int
    k: int
    s: int
    p: int

    @property
    def Ho(self):
        return (self.H + 2 * self.p - self.k) // self.s + 1

    @property
    def Wo(self):
        return (self.W + 2 * self.p - self.k) // self.s + 1

    @property
    def K(self):
        return self.k * self.k * self.cin

    @property
    def M(self):
        return self.B * self.Ho * self.Wo


class Epi(NamedTuple):
    """One epilogue: bias, ReLU, residual add; out = "padded" (one-pixel border), "dense" ([M, C_out]) or "f32" (fp16x2: the
    dense fp32 logit matrix)."""
    bias: bool
    relu: bool
    add: bool
    out: str


EPIS = (Epi(True, True, False, "padded"), Epi(True, True, True, "padded"), Epi(False, False, False, "dense"),
        Epi(True, False, True, "dense"))
EPIS_F16X2 = EPIS + (Epi(True, False, True, "f32"), Epi(False, False, False, "f32"))
# the persistent first-layer kernel has no residual and no fp32 output; the plan sends it dense outputs as well
EPIS_FIRST = (Epi(True, True, False, "padded"), Epi(True, False, False, "padded"), Epi(False, False, False, "padded"),
              Epi(False, False, False, "dense"))


# ---------------------------------------------------------------- operands and the float64 reference
def _coded_x(l, dev):
    """Position-coded input [B, H, W, C] (float64): neighbours along y, x and c differ (asserted)."""
    idx = torch.arange(l.B * l.H * l.W * l.cin, device=dev).view(l.B, l.H, l.W, l.cin)
    if l.mode == "fp32":
        x = (idx + 1).double()                                       # the linear index of (b, y, x, c), plus 1
    elif l.mode == "fp16x2":
        x = ((idx * 2049 + 1) % (1 << 21)).double() / 2048.0         # n / 2048: neighbours differ in the hi AND the lo plane
    else:
        x = ((idx * 37 + (idx // 251) * 11) % 251 - 125).double()    # a small-integer hash in [-125, 125]
    for d in (1, 2, 3):
        assert bool((x.diff(dim=d) != 0).all()), (l, d)
    return x


def _selected_k(l, i):
    """The k = (ky, kx, c) index output channel co selects in launch i: consecutive where all of K can be covered
    (K <= 8 C_out), else in steps of one k-tile plus one (every position of a k-tile, a spread of taps)."""
    step = 1 if l.K <= 8 * l.cout else BK[l.mode] + 1
    return ((torch.arange(l.cout) + i * l.cout) * step) % l.K


def _n_selectors(l, n_epi):
    return max(n_epi, _cdiv(l.K, l.cout) if l.K <= 8 * l.cout else 3)


def _assert_cover(l, n):
    ks = torch.cat([_selected_k(l, i) for i in range(n)])
    assert set((ks // l.cin).tolist()) == set(range(l.k * l.k)), (l, "every (ky, kx)")
    assert set((ks % BK[l.mode]).tolist()) == set(range(min(BK[l.mode], l.K))), (l, "every position of a k-tile")
    if l.K <= 8 * l.cout:
        assert set(ks.tolist()) == set(range(l.K)), (l, "every tap")


def _selector_w(l, i, dev):
    co = torch.arange(l.cout)
    w = torch.zeros((l.cout, l.K), dtype=torch.float64)
    w[co, _selected_k(l, i)] = torch.where((co + i) % 3 == 0, -1.0, 1.0).double()
    return w.to(dev)


def _assert_representable(mode, v):
    """Every value of the float64 reference is exact in the output format (the issue's preconditions)."""
    if mode == "bf16":
        assert torch.equal(v, v.round()) and float(v.abs().max()) <= 256
    elif mode == "fp32":
        assert torch.equal(v, v.round()) and float(v.abs().max()) < 2 ** 24
    else:                                                # hi = fp16(v), lo = fp16((v - hi) * 2048)
        n = v * 2048.0
        assert torch.equal(n, n.round()) and float(n.abs().max()) < 2 ** 22


def _fmt(mode, v):
    """float64 -> the mode's storage with a leading plane axis ([1, ...], fp16x2 [2, ...]); the conversion must be exact."""
    t = v.float()
    if mode == "fp16x2":
        hi = t.half()
        lo = ((t - hi.float()) * 2048.0).half()
        assert torch.equal(hi.double() + lo.double() / 2048.0, v)
        return torch.stack([hi, lo]).contiguous()
    t = t.to(DT[mode])
    assert torch.equal(t.double(), v)
    return t.unsqueeze(0).contiguous()


def _bordered(t, fill):
    """[P, B, h, w, C] -> [P, B, h + 2, w + 2, C] with a border of `fill`"""
    P, B, h, w, C = t.shape
    out = torch.full((P, B, h + 2, w + 2, C), fill, dtype=t.dtype, device=t.device)
    out[:, :, 1:-1, 1:-1] = t
    return out


class Case(NamedTuple):
    """Operands of one launch in the mode's storage and the expected output (`want` [P, B, Ho, Wo, C_out])."""
    x: torch.Tensor
    w: torch.Tensor
    bias: Optional[torch.Tensor]
    add: Optional[torch.Tensor]
    want: torch.Tensor


def _case(l, check, i, e):
    dev = _device()
    co = torch.arange(l.cout, device=dev)
    if check == "sel":
        x, w = _coded_x(l, dev), _selector_w(l, i, dev)
    else:
        g = torch.Generator().manual_seed(7919 * i + 13 * l.K + l.cout)
        x = torch.randint(-1, 2, (l.B, l.H, l.W, l.cin), generator=g).double().to(dev)
        w = torch.randint(-1, 2, (l.cout, l.K), generator=g).double()
        if l.mode == "bf16":                             # thinned: |sum| stays far below 256 (sigma <= 17)
            w = w * (torch.rand((l.cout, l.K), generator=g) < min(1.0, 600.0 / l.K))
        w = w.to(dev)
    frac = l.mode == "fp16x2" and check == "sel"         # multiples of 1 / 2048: the lo planes of bias and residual work too
    bias = add = None
    if e.bias:
        bias = {"bf16": co * 5 % 7 - 3, "fp32": co * 5 % 2001 - 1000,
                "fp16x2": co * 12345 % 16385 - 8192 if frac else co * 5 % 7 - 3}[l.mode].double()
        bias = bias / 2048.0 if frac else bias
    if e.add:
        j = torch.arange(l.M * l.cout, device=dev).view(l.B, l.Ho, l.Wo, l.cout)
        add = {"bf16": j * 37 % 201 - 100, "fp32": j * 7919 % 2001 - 1000,
               "fp16x2": j * 7919 % (1 << 21) - (1 << 20) if frac else j * 37 % 201 - 100}[l.mode].double()
        add = add / 2048.0 if frac else add
    w4 = w.view(l.cout, l.k, l.k, l.cin).permute(0, 3, 1, 2)
    y = F.conv2d(x.permute(0, 3, 1, 2), w4, bias, stride=l.s, padding=l.p).permute(0, 2, 3, 1)
    assert y.shape == (l.B, l.Ho, l.Wo, l.cout) and l.H != l.W and l.Ho != l.Wo
    pre = torch.relu(y) if e.relu else y
    ref = pre + add if e.add else pre
    out_mode = "fp32" if e.out == "f32" else l.mode
    _assert_representable(l.mode, pre)                   # bf16 rounds the convolution before it adds the residual
    _assert_representable(l.mode, ref)
    a = None
    if e.add:
        a = _fmt(l.mode, add)
        a = _bordered(a, float("nan")) if e.out == "padded" else a.view(a.shape[0], l.M, l.cout)
    # the input's border is the zero padding; a layer without padding must never read it
    return Case(_bordered(_fmt(l.mode, x), 0.0 if l.p else float("nan")), _fmt(l.mode, w),
                None if bias is None else bias.float().contiguous(), a, _fmt(out_mode, ref))


def _slice_case(c, n):
    """the first n samples of a case (the convolution is per sample)"""
    return c._replace(x=c.x[:, :n].contiguous(), want=c.want[:, :n].contiguous(),
                      add=None if c.add is None else c.add[:, :n].contiguous())


# ---------------------------------------------------------------- the launch, with canaries
def _canary_buffer(P, numel, guard, dtype):
    """P planes of numel elements, each followed by `guard` elements, everything filled with the canary"""
    buf = torch.empty((P, numel + guard), dtype=dtype, device="cuda")
    buf.view(_INT[dtype]).fill_(CANARY[dtype])
    return buf


def _run(l, c, e, live=None):
    """conv2d_nhwc of layer l on case c with epilogue e (live: n_active of the dynamic-batch call, capacity l.B) into a
    canary-filled buffer.  Asserts that nothing outside the live outputs changed; returns them as [P, n, Ho, Wo, C_out]."""
    from mem_amd import ops
    n = l.B if live is None else live
    f16x2 = l.mode == "fp16x2"
    dt = torch.float32 if e.out == "f32" else DT[l.mode]
    P = 2 if f16x2 and e.out != "f32" else 1
    shape = (l.B, l.Ho + 2, l.Wo + 2, l.cout) if e.out == "padded" else (l.M, l.cout)
    numel = 1
    for d in shape:
        numel *= d
    buf = _canary_buffer(P, numel, 3 * l.cout, dt)       # dense: three extra rows behind the matrix
    out = buf[:, :numel].view((P,) + shape)
    written = torch.zeros(buf.shape, dtype=torch.bool, device="cuda")
    wv = written[:, :numel].view((P,) + shape)
    if e.out == "padded":
        wv[:, :n, 1:-1, 1:-1] = True
    else:
        wv[:, :n * l.Ho * l.Wo] = True
    x, na = c.x, None
    if live is not None:
        x = x.clone()
        x[:, live:] = float("nan")                       # the slots behind the live samples are never read
        na = torch.tensor([live], dtype=torch.int32, device="cuda")

    def arg(t):
        return None if t is None else (t if f16x2 else t[0])
    ops.conv2d_nhwc(arg(x), arg(c.w), c.bias, out if P == 2 else out[0], l.B, l.H, l.W, l.cin, l.cout, l.k, l.s, l.p,
                    relu=e.relu, add=arg(c.add), out_padded=e.out == "padded", n_active=na)
    bits = buf.view(_INT[dt])
    assert bool((bits[~written] == CANARY[dt]).all()), (l, e, live, "a write outside the live outputs")
    if e.out == "padded":
        return out[:, :n, 1:-1, 1:-1]
    return out[:, :n * l.Ho * l.Wo].view(P, n, l.Ho, l.Wo, l.cout)


def _plan(l, e, dynamic=False):
    from mem_amd import ops
    return ops.conv_plan(l.mode, l.B, l.H, l.W, l.cin, l.cout, l.k, l.s, l.p, add=e.add, out_f32=e.out == "f32",
                         out_padded=e.out == "padded", dynamic=dynamic)


def _assert_static_plan(l, epis, name, tile_m=TILE_M):
    """every epilogue of the layer plans onto `name`, one tile per workgroup"""
    for e in epis:
        plan = _plan(l, e)
        (got, grid, *_), = plan.launches
        assert got == name and grid == _cdiv(l.M, tile_m) * _cdiv(l.cout, TILE_N), (l, e, plan.launches)
        assert (plan.Hp, plan.Wp, plan.Ho, plan.Wo, plan.K, plan.M) == (l.H + 2, l.W + 2, l.Ho, l.Wo, l.K, l.M)


def _exact_checks(l, epis, memo, live=None, checks=("sel", "int")):
    """Both exact checks on layer l, the epilogues taking turns over the launches.  memo: the cases (reference computed once,
    shared between the kernel forms of a test).  Returns {(check, launch): live outputs}."""
    outs = {}
    for check in checks:
        n = _n_selectors(l, len(epis)) if check == "sel" else len(epis)
        if check == "sel":
            _assert_cover(l, n)
        for i in range(n):
            e = epis[i % len(epis)]
            key = (l, check, i, e)
            if key not in memo:
                memo[key] = _case(*key)
            c = memo[key]
            got = _run(l, c, e, live)
            assert torch.equal(got, c.want[:, :got.shape[1]]), (l, check, i, e, live)
            outs[(check, i)] = got
    return outs


def _assert_bit_equal(a, b, n=None):
    assert a.keys() == b.keys()
    for key in a:
        x, y = a[key][:, :n], b[key][:, :n]
        assert torch.equal(x.contiguous().view(_INT[x.dtype]), y.contiguous().view(_INT[y.dtype])), key


# ---------------------------------------------------------------- 1. exact layer checks, form by form
@pytest.mark.parametrize("l", [Layer("bf16", 5, 10, 14, 4, 72, 4, 2, 1),          # first layer: C_in = 4, M = 175
                               Layer("bf16", 3, 6, 10, 64, 72, 3, 1, 1),          # M = 180
                               Layer("bf16", 3, 5, 9, 128, 72, 3, 1, 1),          # K = 1152 > 8 C_out
                               Layer("bf16", 3, 6, 10, 64, 72, 1, 1, 0),
                               Layer("bf16", 3, 5, 9, 128, 136, 1, 1, 0)],        # two column tiles, the second of 8 columns
                         ids=lambda l: "k%ds%d_c%d_o%d" % (l.k, l.s, l.cin, l.cout))
def test_bf16_conv_exact(l):
    """csrc/conv.hip::conv_gemm_kernel: 4x4/s2 on the four-channel first layer, 3x3/s1 and 1x1 with C_in = 64 and 128;
    C_out = 72 (ragged column tile, a multiple of 8), M not a multiple of 128 and above 128 (two row tiles)."""
    assert l.M % TILE_M and l.M > TILE_M and l.cout % TILE_N
    _assert_static_plan(l, EPIS, "conv_gemm_kernel")
    _exact_checks(l, EPIS, {})


@pytest.mark.parametrize("l", [Layer("fp32", 3, 10, 14, 8, 12, 2, 2, 0),          # K = 32: a single k-tile; M = 105
                               Layer("fp32", 3, 7, 11, 32, 132, 3, 1, 1),         # K = 288, two column tiles; M = 231
                               Layer("fp32", 5, 10, 14, 12, 20, 4, 2, 1),         # K = 192: a k-tile spans 2 2/3 taps; M = 175
                               Layer("fp32", 3, 5, 9, 96, 200, 1, 1, 0),          # K = 96; M = 135
                               Layer("fp32", 2, 11, 17, 32, 12, 3, 3, 1)],        # stride 3: 4 x 6 outputs; K = 288 > 8 C_out
                         ids=lambda l: "k%ds%dp%d_c%d_o%d" % (l.k, l.s, l.p, l.cin, l.cout))
def test_f32_static_conv_exact(l):
    """csrc/conv_f32.hip::conv_gemm_f32_kernel, static batch: 2x2/s2/p0, 3x3/s1/p1, 4x4/s2/p1, 1x1, stride 3 once; C_in and
    C_out multiples of 4 but not of 64; K = 32 and K >= 96."""
    assert l.cin % 64 and l.cout % 64
    _assert_static_plan(l, EPIS, "conv_gemm_f32_kernel")
    _exact_checks(l, EPIS, {})


def _dynamic_plan(l, e):
    """The two launches of a dynamic-batch call: (grid of the 32-row form, grid of the 128-row form, switch count).  Their
    live-count ranges partition [0, 2^30)."""
    (n0, g0, _, _, lo0, hi0), (n1, g1, _, _, lo1, hi1) = _plan(l, e, dynamic=True).launches
    assert (n0, n1) == ("conv_gemm_f32_m32_kernel", "conv_gemm_f32_kernel")
    assert lo0 == 0 and hi0 == lo1 and hi1 == 1 << 30
    ntn = _cdiv(l.cout, TILE_N)
    assert g0 == min(2048, _cdiv(l.M, SMALL_M) * ntn) and g1 == min(1024, _cdiv(l.M, TILE_M) * ntn)
    return g0, g1, hi0


@pytest.mark.parametrize("l", [Layer("fp32", 3, 6, 10, 32, 40, 3, 1, 1), Layer("fp32", 3, 10, 14, 12, 20, 4, 2, 1)],
                         ids=lambda l: "k%ds%d" % (l.k, l.s))
def test_f32_dynamic_m32_spatial_taps(l):
    """conv_gemm_f32_m32_kernel has its own gather arithmetic: 3x3/s1 and 4x4/s2 with H != W through the dynamic-batch call at
    0, 1 and 2 live samples of a capacity of 3 (all below the switch count: the 32-row form works, the 128-row launch writes
    nothing).  Exact against float64, live slots equal to the static result bit for bit, slots behind them untouched."""
    memo = {}
    for e in EPIS:
        _, _, sw = _dynamic_plan(l, e)
        assert sw > l.B
    static = _exact_checks(l, EPIS, memo)
    for live in (0, 1, 2):
        _assert_bit_equal(_exact_checks(l, EPIS, memo, live=live), static, live)


def test_f32_dynamic_clamped_grids_and_switch():
    """The two persistent forms of the dynamic-batch call where their grids are clamped and workgroups walk more than one tile.
    conv_plan switches to the 128-row form at sw = ceil(512 * 128 / (Ho Wo ntn)) live samples, so the 32-row form never sees
    more than (sw - 1) Ho Wo < 65536 / ntn live rows, i.e. fewer than 2048 + ntn tiles: a second tile per workgroup is only
    reachable with many column tiles.  1x1, C_in = 32, C_out = 8060 (ntn = 63, the last tile of 124 columns), 8 x 13 pixels:
    sw = 11, and at 10 live samples the 32-row form has 33 * 63 = 2079 live tiles on its 2048 workgroups (31 walk two tiles,
    2017 one).  Capacity 12: grid of the 128-row form 630 < 1024 (live = sw and live = capacity); capacity 20: 17 * 63 = 1071
    tiles on 1024 workgroups at live = capacity (47 walk two).  Live counts 0, 1, sw - 1 (32-row form; the 128-row launch must
    write nothing: the result is the exact one and the canary behind it is intact), sw and the capacity (128-row form).  Every
    result is exact against float64 and its live slots equal the static call's bit for bit.
    (The certified-tokenizer tests never reach the 128-row form with n_active: the switch counts of their small configs are
    far above their capacities; test_tokenizer_nonsquare_certified asserts the counts of its config from the plan.)"""
    for cap, epis in ((12, (Epi(True, True, True, "padded"), Epi(False, False, False, "dense"))),
                      (20, (Epi(True, False, True, "dense"),))):
        l = Layer("fp32", cap, 8, 13, 32, 8060, 1, 1, 0)
        ntn, hw = _cdiv(l.cout, TILE_N), l.Ho * l.Wo
        for e in epis:
            g32, g128, sw = _dynamic_plan(l, e)
        assert ntn == 63 and sw == _cdiv(512 * TILE_M, hw * ntn) == 11 and sw < cap
        assert g32 == 2048 < _cdiv(l.M, SMALL_M) * ntn                       # clamped
        tiles32 = _cdiv((sw - 1) * hw, SMALL_M) * ntn
        assert g32 < tiles32 < 2 * g32                                      # workgroups walk 2 tiles or 1
        if cap == 12:
            assert g128 == _cdiv(l.M, TILE_M) * ntn < 1024
        else:
            assert g128 == 1024 < _cdiv(l.M, TILE_M) * ntn < 2 * 1024       # at live = capacity: 2 tiles or 1
        print(f"capacity {cap}: switch {sw}; 32-row grid {g32} for {tiles32} tiles at {sw - 1} live; 128-row grid {g128} for "
              f"{_cdiv(sw * hw, TILE_M) * ntn} tiles at {sw} live, {_cdiv(l.M, TILE_M) * ntn} at {cap}")
        memo = {}
        static = _exact_checks(l, epis, memo)
        for live in ((0, 1, sw - 1, sw, cap) if cap == 12 else (sw - 1, sw, cap)):
            _assert_bit_equal(_exact_checks(l, epis, memo, live=live), static, live)
        del memo, static


def test_f32_dynamic_128_row_spatial_taps_every_epilogue():
    """The 128-row form under n_active on a layer with nine taps, through every epilogue at one size: 3x3/s1/p1 on 6 x 10,
    C_in = 32, C_out = 2040 (16 column tiles, the last of 120 columns) -- that many channels bring the switch count (69) below
    a capacity (70) whose outputs stay at 55 MB.  Live = switch and live = capacity run the 128-row form (grid 528 = its tiles
    at the capacity), live = switch - 1 the 32-row form on exactly its 2048 workgroups.  Exact against float64, live slots
    equal to the static result bit for bit, slots behind them untouched."""
    l = Layer("fp32", 70, 6, 10, 32, 2040, 3, 1, 1)
    ntn, hw = _cdiv(l.cout, TILE_N), l.Ho * l.Wo
    for e in EPIS:
        g32, g128, sw = _dynamic_plan(l, e)
    assert sw == _cdiv(512 * TILE_M, hw * ntn) == 69 < l.B
    assert g128 == _cdiv(l.M, TILE_M) * ntn == 528 and g32 == 2048 == _cdiv((sw - 1) * hw, SMALL_M) * ntn
    memo = {}
    static = _exact_checks(l, EPIS, memo)
    for live in (sw - 1, sw, l.B):
        _assert_bit_equal(_exact_checks(l, EPIS, memo, live=live), static, live)


@pytest.mark.parametrize("l", [Layer("fp16x2", 3, 9, 13, 64, 192, 3, 1, 1), Layer("fp16x2", 3, 9, 13, 64, 192, 1, 1, 0)],
                         ids=lambda l: "k%d" % l.k)
def test_f16x2_tile_forms_exact_and_bit_equal(l):
    """conv_gemm_f16x2_kernel<8>, <4> (conv_waves 8 and 4) and conv_gemm_f16x2_wide_kernel (conv_waves 32): 3x3 and 1x1,
    C_in = 64, C_out = 192 (1.5 column tiles), M = 351 (ragged for the 128-row and for the 256-row tile); every epilogue
    including the dense fp32 logit output.  Exact against float64, and the three forms bit-equal."""
    from mem_amd import _lib
    assert l.M % TILE_M and l.M % WIDE_M
    memo, outs = {}, {}
    waves0 = _lib.get_option("conv_waves")
    try:
        for waves, name, tile_m in ((8, "conv_gemm_f16x2_kernel<8>", TILE_M), (4, "conv_gemm_f16x2_kernel<4>", TILE_M),
                                    (32, "conv_gemm_f16x2_wide_kernel", WIDE_M)):
            _lib.set_option("conv_waves", waves)
            _assert_static_plan(l, EPIS_F16X2, name, tile_m)
            outs[waves] = _exact_checks(l, EPIS_F16X2, memo)
    finally:
        _lib.set_option("conv_waves", waves0)
    _assert_bit_equal(outs[4], outs[8])
    _assert_bit_equal(outs[32], outs[8])


def _first_layer_cols(cout):
    """workgroups per column tile of the persistent first-layer kernel on this device, from the plan of a layer with more row
    tiles than any device has CUs"""
    big = Layer("fp16x2", 1 << 12, 16, 32, 4, cout, 4, 2, 1)
    (name, grid, *_), = _plan(big, EPIS_FIRST[0]).launches
    assert name == "conv_gemm_f16x2_first_kernel" and grid % (cout // TILE_N) == 0
    return grid // (cout // TILE_N)


def test_f16x2_first_layer_one_tile_and_its_fallbacks():
    """conv_gemm_f16x2_first_kernel (persistent; default conv_waves, C_in = 4, 4x4/s2, no add, padded output, whole tiles):
    (a) one tile: B = 1, 16 x 32 input, C_out = 128.
    (c) the same layer with a residual plans onto <8> and, with a zero residual, gives the first-layer kernel's bits; the same
        layer on 14 x 32 images takes the first-layer kernel at B = 8 (M = 896 = 7 tiles) and <8> at B = 3 (M = 336, ragged):
        the three shared samples are bit-equal.  The residual and fp32-output epilogues of the four-channel layer run on <8>,
        exactly."""
    from mem_amd import _lib
    assert _lib.get_option("conv_waves") == 16
    memo = {}
    la = Layer("fp16x2", 1, 16, 32, 4, 128, 4, 2, 1)
    assert la.M == TILE_M
    for e in EPIS_FIRST:
        (name, grid, *_), = _plan(la, e).launches
        assert name == "conv_gemm_f16x2_first_kernel" and grid == 1
    first = _exact_checks(la, EPIS_FIRST, memo)
    rest = tuple(e for e in EPIS_F16X2 if e.add or e.out == "f32")
    _assert_static_plan(la, rest, "conv_gemm_f16x2_kernel<8>")
    _exact_checks(la, rest, memo)
    e0, e_add = EPIS_FIRST[0], Epi(True, True, True, "padded")
    for check in ("sel", "int"):
        c = memo[(la, check, 0, e0)]
        z = c._replace(add=torch.zeros((2, la.B, la.Ho + 2, la.Wo + 2, la.cout), dtype=torch.float16, device="cuda"))
        _assert_bit_equal({0: _run(la, z, e_add)}, {0: first[(check, 0)]})
    l8, l3 = Layer("fp16x2", 8, 14, 32, 4, 128, 4, 2, 1), Layer("fp16x2", 3, 14, 32, 4, 128, 4, 2, 1)
    assert l8.M % TILE_M == 0 and l3.M % TILE_M
    cols = _first_layer_cols(128)
    for e in EPIS_FIRST:
        (name, grid, *_), = _plan(l8, e).launches
        assert name == "conv_gemm_f16x2_first_kernel" and grid == min(cols, l8.M // TILE_M)
    _assert_static_plan(l3, EPIS_FIRST, "conv_gemm_f16x2_kernel<8>")
    memo = {}
    whole = _exact_checks(l8, EPIS_FIRST, memo)
    for (ll, check, i, e), c in list(memo.items()):
        got = _run(l3, _slice_case(c, 3), e)
        assert torch.equal(got, c.want[:, :3])
        _assert_bit_equal({0: got}, {0: whole[(check, i)]}, 3)


def test_f16x2_first_layer_walks_two_and_three_tiles():
    """(b) C_out = 256 and 2.5 x as many whole row tiles as the plan gives a column tile workgroups (the count comes from the
    plan query, not from a CU number written here): the grid is smaller than the tile count and does not divide it, so the
    persistent workgroups walk 2 and 3 row tiles -- the counted waits see a previous tile's stores in flight."""
    cout, full = 256, 2
    cols = _first_layer_cols(cout)
    nmt = 2 * cols + max(cols // 2, 1)
    l = Layer("fp16x2", nmt, 16, 32, 4, cout, 4, 2, 1)                      # 8 x 16 = 128 output pixels per sample
    assert l.M == nmt * TILE_M
    epis = (EPIS_FIRST[0], EPIS_FIRST[2])
    for e in epis:
        (name, grid, *_), = _plan(l, e).launches
        assert name == "conv_gemm_f16x2_first_kernel" and grid == cols * full
        assert grid < nmt * full and nmt % cols != 0 and 2 * cols < nmt < 3 * cols
    print(f"first layer, C_out {cout}: grid {cols * full} workgroups for {nmt * full} tiles ({nmt} row tiles per column tile)")
    _exact_checks(l, epis, {})


# ---------------------------------------------------------------- 2. layout and certification plumbing
def _normalised(x, mean, std):
    """(x - mean) / std as the kernels compute it: an fp32 subtraction, then an fp32 division (csrc/*.hip:
    `u = (u - mean[c]) / stdv[c]`, built with -fno-fast-math: no reciprocal), each correctly rounded -- mirrored as
    float64-then-fp32 per operation, which rounds once (a 53-bit intermediate of a 24-bit operation)."""
    d = (x.double() - mean.double().view(1, -1, 1, 1)).float()
    return (d.double() / std.double().view(1, -1, 1, 1)).float()


MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16x2"])
def test_nchw_to_padded_nhwc4(mode):
    """memhip_nchw_to_padded_nhwc4, B = 2, 6 x 10, C = 1, 3, 4, with and without mean / std.  The kernels only move data and
    apply two correctly rounded fp32 operations, so the interior is compared at rtol = 0, atol = 0 against the float64
    permute; channels C .. 3 of every interior pixel are written as zero (memhip.h: "3 channels + 1 zero" -- the kernels store
    all four channels of a pixel at once); the border and the bytes behind every plane keep the canary.  fp16x2: the planes
    are hi = fp16(v), lo = fp16((v - hi) * 2048) bit for bit, and hi + lo / 2048 reproduces v to 2^-22 relative."""
    from mem_amd import ops
    B, H, W = 2, 6, 10
    dt, P = DT[mode], 2 if mode == "fp16x2" else 1
    g = torch.Generator().manual_seed(17)
    for C in (1, 3, 4):
        for norm in (False, True):
            x = torch.rand((B, C, H, W), generator=g).cuda()
            mean = torch.tensor(MEAN[:C], device="cuda") if norm else None
            std = torch.tensor(STD[:C], device="cuda") if norm else None
            v = _normalised(x, mean, std) if norm else x
            want = torch.zeros((B, H, W, 4), device="cuda")
            want[..., :C] = v.permute(0, 2, 3, 1)
            numel = B * (H + 2) * (W + 2) * 4
            buf = _canary_buffer(P, numel, 64, dt)
            out = buf[:, :numel].view(P, B, H + 2, W + 2, 4)
            ops.nchw_to_padded_nhwc4(x, out if P == 2 else out[0], mean, std)
            written = torch.zeros(buf.shape, dtype=torch.bool, device="cuda")
            written[:, :numel].view(out.shape)[:, :, 1:-1, 1:-1] = True
            assert bool((buf.view(_INT[dt])[~written] == CANARY[dt]).all()), (C, norm)
            got = out[:, :, 1:-1, 1:-1]
            if mode == "fp16x2":
                hi = want.half()
                lo = ((want - hi.float()) * 2048.0).half()
                assert torch.equal(got[0], hi) and torch.equal(got[1], lo), (C, norm)
                back = got[0].double() + got[1].double() / 2048.0
                assert bool(((back - want.double()).abs() <= 2.0 ** -22 * want.double().abs()).all())
            else:
                assert torch.equal(got[0], want.to(dt)), (C, norm)
            assert bool((got[..., C:] == 0).all())


def test_tok_gather_images():
    """memhip_tok_gather_images_f32 on 6 x 10 images: a list with repeats and out of order, count below and above R, offset > 0;
    n_round = clamp(count - offset, 0, R) including 0; slot j holds image list[offset + j] (exact: a gather, or the two fp32
    operations of _normalised); slots at or behind n_round, every border and the bytes behind the buffer keep the canary."""
    from mem_amd import ops
    H, W, R = 6, 10, 3
    g = torch.Generator().manual_seed(23)
    lst = torch.tensor([5, 2, 5, 0, 6, 2, 1, 5], dtype=torch.int32, device="cuda")
    for C, norm in ((3, True), (3, False), (1, False), (4, True)):
        x = torch.rand((7, C, H, W), generator=g).cuda()
        mean = torch.tensor(MEAN[:C], device="cuda") if norm else None
        std = torch.tensor(STD[:C], device="cuda") if norm else None
        v = _normalised(x, mean, std) if norm else x
        for count, off in ((2, 0), (8, 0), (5, 3), (8, 5), (7, 6), (3, 3), (2, 4)):
            live = max(0, min(R, count - off))
            numel = R * (H + 2) * (W + 2) * 4
            buf = _canary_buffer(1, numel, 64, torch.float32)
            out = buf[0, :numel].view(R, H + 2, W + 2, 4)
            n_round = torch.full((1,), -7, dtype=torch.int32, device="cuda")
            cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
            ops.tok_gather_images(x, mean, std, lst, cnt, off, R, out, n_round)
            assert int(n_round.item()) == live, (count, off)
            want = torch.zeros((live, H, W, 4), device="cuda")
            want[..., :C] = v[lst[off:off + live].long()].permute(0, 2, 3, 1)
            assert torch.equal(out[:live, 1:-1, 1:-1], want), (C, norm, count, off)
            written = torch.zeros(buf.shape, dtype=torch.bool, device="cuda")
            written[0, :numel].view(out.shape)[:live, 1:-1, 1:-1] = True
            assert bool((buf.view(torch.int32)[~written] == CANARY[torch.float32]).all()), (C, norm, count, off)


def test_tok_scatter_ids():
    """memhip_tok_scatter_ids with 24 and 70 tokens per sample (not multiples of 64): n_round = 0, 1 and R; row list[offset + j]
    of ids_out takes slot j of ids_in, no other row changes."""
    from mem_amd import ops
    R, B = 3, 9
    lst = torch.tensor([7, 4, 8, 1, 6, 0, 3], dtype=torch.int32, device="cuda")
    for hw in (24, 70):
        ids_in = (torch.arange(R * hw, device="cuda") * 3 + 1000).to(torch.int64)
        for n, off in ((0, 0), (1, 2), (R, 0), (R, 4), (2, 5)):
            init = -1 - torch.arange(B * hw, device="cuda").to(torch.int64)
            ids_out = init.clone()
            ops.tok_scatter_ids(ids_in, lst, torch.tensor([n], dtype=torch.int32, device="cuda"), off, R, hw, ids_out)
            want = init.clone().view(B, hw)
            for j in range(n):
                want[int(lst[off + j])] = ids_in[j * hw:(j + 1) * hw]
            assert torch.equal(ids_out.view(B, hw), want), (hw, n, off)


# ---------------------------------------------------------------- 3. a non-square tokenizer, end to end
NS = dict(input_H=64, input_W=96, num_tokens=512, codebook_dim=64, num_layers=4, num_resnet_blocks=1, hidden_dim=64, channels=3,
          normalization=((0.5, 0.45, 0.55), (0.25, 0.2, 0.3)))


def _ns_vae(seed, dev):
    """The module with labels that DEPEND ON THE PIXELS: at the default initialisation the head's bias decides the argmax (one
    label for every token and every image), so the convolution weights are doubled, the head's bias is zero and the input is
    normalised to both signs."""
    from mem_amd.vae_model import DiscreteVAE
    torch.manual_seed(seed)
    vae = DiscreteVAE(**NS).eval()
    with torch.no_grad():
        for m in vae.encoder.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.mul_(2.0)
        vae.encoder[-1].bias.zero_()
    return vae.to(dev)


def _ns_images(seed, n, dev):
    """noise under a brightness of its own per 16 x 16 block and channel (one block per final token): the tokens differ"""
    g = torch.Generator().manual_seed(seed)
    H, W = NS["input_H"], NS["input_W"]
    u = torch.rand((n, 3, H, W), generator=g)
    blk = torch.rand((n, 3, H // 16, W // 16), generator=g)
    return (u * F.interpolate(blk, scale_factor=16, mode="nearest")).to(dev)


def _labels64(vae, img):
    """(float64 logits [B, hw, tokens], labels) of the torch module"""
    lg = vae.double()(img.double(), return_logits=True).flatten(2).transpose(1, 2)
    vae.float()
    return lg, lg.argmax(-1)


@pytest.mark.parametrize("precision", ["fp32", "fp16x2", "bf16"])
def test_tokenizer_nonsquare_all_precisions(precision):
    """64 x 96 images (final map 4 x 6), hidden 64, 512 tokens, 1 ResBlock, 4 layers, 8 images, with mean / std, against the
    float64 evaluation of the same torch module.  The reference must be worth comparing with: its labels depend on the pixels
    -- at least 30 distinct labels among the 192 tokens, and more than half of them change when the image memory is read as
    96 x 64 (transposed) or the image is shifted by one pixel in x; asserted before the comparison (float64 on the CPU for this
    seed: 43 distinct labels, 77 % differ transposed, 72 % shifted).  fp32 and fp16x2: the rule of
    test_tokenizer_fp32_equals_fp64_module -- labels equal wherever the float64 top-2 gap exceeds 1e-4 of the logit spread, and
    more than 0.99 of the tokens are that safe (a cap on what the test may leave out; on the CPU for this seed all 192 are, the
    smallest gap is 6.3e-4 of the spread).  bf16: the rule of test_tokenizer_agreement_with_fp32_module."""
    from mem_amd.vae_model import HipTokenizer
    vae = _ns_vae(1, "cuda")
    img = _ns_images(1, 8, "cuda")
    tok = HipTokenizer(vae, max_batch=8, precision=precision, certify=False)
    assert (tok.H, tok.W, tok.hw_out) == (64, 96, (4, 6)) and tok.norm is not None
    ids = tok.get_codebook_indices(img)
    assert ids.shape == (8, 24) and ids.dtype == torch.int64
    lg, ref = _labels64(vae, img)
    swapped = _labels64(vae, img.transpose(-1, -2).reshape(img.shape))[1]
    shifted = _labels64(vae, torch.roll(img, 1, dims=-1))[1]
    distinct = ref.unique().numel()
    print(f"float64 reference: {distinct} distinct labels; {(swapped != ref).float().mean().item():.2f} differ on the transposed, "
          f"{(shifted != ref).float().mean().item():.2f} on the shifted image")
    assert distinct >= 30
    assert (swapped != ref).float().mean().item() > 0.5 and (shifted != ref).float().mean().item() > 0.5
    if precision == "bf16":
        ref = vae.get_codebook_indices(img)
        lg = vae(img, return_logits=True).flatten(2).transpose(1, 2)
        gap = (lg.gather(2, ref.unsqueeze(-1)) - lg.gather(2, ids.unsqueeze(-1))).squeeze(-1)
        spread = lg.std().item()
        agree = (ids == ref).float().mean().item()
        print(f"bf16: agreement {agree:.4f}, largest gap {gap.max().item():.3e}, spread {spread:.3f}")
        assert agree >= 0.97, agree
        assert gap.max().item() <= 0.05 * spread + 1e-3, (gap.max().item(), spread)
        return
    top2 = lg.topk(2, dim=-1).values
    safe = (top2[..., 0] - top2[..., 1]) > 1e-4 * lg.std()
    assert safe.float().mean().item() > 0.99
    assert torch.equal(ids[safe], ref[safe])


def test_tokenizer_nonsquare_certified():
    """The certified fp16x2 path at 64 x 96 with planted near-ties (test_certified_tokenizer_planted_near_ties at this config:
    the upper half of the classes are copies of the lower half perturbed by 1e-5 relative, so nearly every token is a near-tie
    between a class and its twin -- asserted on the fp32 gaps as there): every one of the 12 samples is flagged and goes
    through tok_gather_images, the dynamic-batch fp32 walk and tok_scatter_ids with H != W in three rounds of 4 (offsets 0, 4,
    8); the ids equal the fp32 mode's on every token.  The fp32 mode is itself held to the float64 module on this model and
    these images before it serves as the reference (safe-token rule with the twins folded into one label; float64 on the CPU
    for this seed: 36 distinct labels, all 288 tokens safe, the smallest gap 8.4e-4 of the spread).  Every layer of the recompute
    stays on the 32-row form: the switch counts of this config, from the plan, are 43 .. 2731 against a capacity of 4."""
    from mem_amd import ops
    from mem_amd.vae_model import HipTokenizer
    vae = _ns_vae(1, "cpu")
    head = vae.encoder[-1]
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        head.weight[256:] = head.weight[:256] * (1.0 + 1e-5 * torch.randn(head.weight[:256].shape, generator=g))
    vae = vae.cuda()
    B, R = 12, 4
    img = _ns_images(3, B, "cuda")
    t32 = HipTokenizer(vae, max_batch=B)
    ids32 = t32.get_codebook_indices(img).clone()
    gap32 = t32.last_top2_gap(B)
    rms = t32.logits.float().pow(2).mean(1).sqrt().view(B, -1)
    rel = (gap32 / rms).flatten()
    assert (rel < 7e-5).float().mean() > 0.8 and rel.min() < 1e-6 and rel.max() > 1e-7, (rel.min(), rel.median(), rel.max())
    # the reference of this test against the torch module: twins folded (class c and c + 256 are one label up to the near-tie)
    lg, ref = _labels64(vae, img)
    pair = torch.maximum(lg[..., :256], lg[..., 256:])
    top2 = pair.topk(2, dim=-1).values
    safe = (top2[..., 0] - top2[..., 1]) > 1e-4 * lg.std()
    assert safe.float().mean().item() > 0.99 and (ref % 256).unique().numel() >= 30
    assert torch.equal((ids32 % 256)[safe], (ref % 256)[safe])
    cert = HipTokenizer(vae, max_batch=B, precision="fp16x2", exact_capacity=R)
    ex = cert._exact
    assert ex.max_batch == R and (ex.H, ex.W, ex.hw_out) == (64, 96, (4, 6))
    h, w, switch = ex.H, ex.W, []
    for kind, L in ex.layers:
        for c in (L if kind == "res" else (L,)):
            plan = ops.conv_plan("fp32", R, h, w, c.cin, c.cout, c.k, c.stride, c.pad, add=c is L[-1] if kind == "res" else False,
                                 out_padded=kind != "head", dynamic=True)
            assert plan.launches[0][0] == "conv_gemm_f32_m32_kernel"
            switch.append(plan.launches[0][5])
            h, w = c.out_hw(h, w)
    assert switch == [43, 171, 683, 2731, 2731, 2731, 2731, 683] and min(switch) > R
    ids = cert.get_codebook_indices(img)
    st = cert.certification_stats()
    print(f"non-square planted near-ties: flagged samples {st}")
    assert st["flagged_samples"] == B > R and st["calls"] == 1
    assert torch.equal(ids, ids32)
    assert torch.equal(cert.get_codebook_indices(img[5:11]), ids32[5:11])
