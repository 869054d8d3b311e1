"""-m "not gpu": the dispatch of the tokenizer convolutions (memhip_conv2d_nhwc, one memhip_conv_args_t for the bf16 / fp32 /
fp32 dynamic / fp16x2 calls), checked through the plan query memhip_conv_plan.  The query takes the struct of the call (ops.conv_plan
builds it), validates and plans like the call itself and launches nothing."""
from collections import Counter

import numpy as np
import pytest

BF16, F32, F32M32, W4, W8, WIDE, FIRST = ("conv_gemm_kernel", "conv_gemm_f32_kernel", "conv_gemm_f32_m32_kernel",
                                          "conv_gemm_f16x2_kernel<4>", "conv_gemm_f16x2_kernel<8>", "conv_gemm_f16x2_wide_kernel",
                                          "conv_gemm_f16x2_first_kernel")
ALL = 1 << 30          # dyn_hi of a launch that works for every live-sample count
KMAX = 160 * 1024      # LDS bytes a workgroup may use


@pytest.fixture(scope="module")
def ops():
    from mem_amd import ops
    return ops


@pytest.fixture
def waves():
    """set(conv_waves); the default 16 comes back afterwards."""
    from mem_amd import _lib
    yield lambda v: _lib.set_option("conv_waves", v)
    _lib.set_option("conv_waves", 16)


# ---------------------------------------------------------------------------------------------------------------------------
# The three launchers of commit a9a608d (memhip_conv2d_nhwc_bf16 in conv.hip, conv2d_nhwc_f32_impl in conv_f32.hip,
# memhip_conv2d_nhwc_f16x2 in conv_f16x2.hip), transcribed statement by statement.  Return None where that code answered
# MEMHIP_EINVAL, else ((Ho, Wo, K, M), launches); launches = [(kernel, grid, workgroup, LDS bytes, dyn_lo, dyn_hi)].
def idiv(a, b):
    """C's integer division (towards zero)."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def cdiv(a, b):
    return (a + b - 1) // b


def encoder_shape(k, s, p):
    return (k, s, p) in ((4, 2, 1), (3, 1, 1), (1, 1, 0))


def parent_bf16(B, H, W, Cin, Cout, k, s, p, add, out_padded):
    BM = BN = 128
    BK = 64
    kStageBytes = 2 * (BM * BK * 2)
    if not (B >= 0 and H > 0 and W > 0 and Cin > 0 and Cout > 0):
        return None
    if B == 0:
        return (0, 0, 0, 0), []
    if not encoder_shape(k, s, p):
        return None
    cin4 = Cin == 4
    if not ((k == 4) if cin4 else (Cin % 64 == 0)):
        return None
    if Cout % 8:
        return None
    Ho, Wo, K = idiv(H + 2 * p - k, s) + 1, idiv(W + 2 * p - k, s) + 1, k * k * Cin
    if K % BK:
        return None
    M = B * Ho * Wo
    if not M < (1 << 31):
        return None
    grid = cdiv(M, BM) * cdiv(Cout, BN)
    return (Ho, Wo, K, M), [(BF16, grid, 256, 2 * kStageBytes, 0, ALL)]


def parent_f32(B, H, W, Cin, Cout, k, s, p, add, out_padded, n_active):
    BM = BN = 128
    BK, SBM = 32, 32
    PITCH = BK + 2
    kTileFloats = BM * PITCH
    kStageFloats = 2 * kTileFloats
    if not (B >= 0 and H > 0 and W > 0 and Cin > 0 and Cout > 0):
        return None
    if B == 0:
        return (0, 0, 0, 0), []
    if not (1 <= k <= 4 and s >= 1 and 0 <= p <= 1):
        return None
    if Cin % 4 or Cout % 4:
        return None
    Ho, Wo, K = idiv(H + 2 * p - k, s) + 1, idiv(W + 2 * p - k, s) + 1, k * k * Cin
    if not (Ho > 0 and Wo > 0):
        return None
    if K % BK:
        return None
    M = B * Ho * Wo
    if not M < (1 << 31):
        return None
    lds = 2 * kStageFloats * 4
    if n_active:
        ntn_, hw_ = cdiv(Cout, BN), Ho * Wo
        kDynSwitch = (512 * BM + hw_ * ntn_ - 1) // (hw_ * ntn_)
        kDynSwitch = 1 if kDynSwitch < 1 else kDynSwitch
        lds_s = 2 * (SBM * PITCH + kTileFloats) * 4
        grid_s = cdiv(M, SBM) * cdiv(Cout, BN)
        grid_s = 2048 if grid_s > 2048 else grid_s
        grid_b = cdiv(M, BM) * cdiv(Cout, BN)
        grid_b = 1024 if grid_b > 1024 else grid_b
        return (Ho, Wo, K, M), [(F32M32, grid_s, 256, lds_s, 0, kDynSwitch), (F32, grid_b, 256, lds, kDynSwitch, ALL)]
    grid = cdiv(M, BM) * cdiv(Cout, BN)
    return (Ho, Wo, K, M), [(F32, grid, 256, lds, 0, ALL)]


def parent_f16x2(B, H, W, Cin, Cout, k, s, p, add, out_padded, out_f32, conv_waves, max_cus):
    BM = BN = 128
    BK = 64
    kTileBytes = BM * BK * 2
    kStageBytes = 4 * kTileBytes
    WBM, WBN, WBK = 256, 128, 32
    kWStage = 2 * (WBM * WBK * 2) + 2 * (WBN * WBK * 2)
    if not (B >= 0 and H > 0 and W > 0 and Cin > 0 and Cout > 0):
        return None
    if B == 0:
        return (0, 0, 0, 0), []
    if not encoder_shape(k, s, p):
        return None
    cin4 = Cin == 4
    if not ((k == 4) if cin4 else (Cin % 64 == 0)):
        return None
    if Cout % 8:
        return None
    if out_f32 and out_padded:
        return None
    Ho, Wo, K = idiv(H + 2 * p - k, s) + 1, idiv(W + 2 * p - k, s) + 1, k * k * Cin
    if K % BK:
        return None
    M = B * Ho * Wo
    if not M < (1 << 31):
        return None
    grid = cdiv(M, BM) * cdiv(Cout, BN)
    wgrid = cdiv(M, WBM) * cdiv(Cout, WBN)
    if cin4 and conv_waves >= 16 and K == BK and not add and not out_f32 and M % BM == 0 and Cout % BN == 0:
        ntn = Cout // BN
        cols = max_cus // ntn
        cols = 1 if cols < 1 else cols
        nmt = M // BM
        cols = nmt if cols > nmt else cols
        kFirstLds = 2 * kTileBytes + 2 * 2 * kTileBytes + 8 * 16 * 72 * 4
        return (Ho, Wo, K, M), [(FIRST, cols * ntn, 512, kFirstLds, 0, ALL)]
    if not cin4 and (conv_waves == 32 or (conv_waves == 16 and wgrid >= 2 * max_cus)):
        return (Ho, Wo, K, M), [(WIDE, wgrid, 512, 3 * kWStage, 0, ALL)]
    if conv_waves == 4:
        return (Ho, Wo, K, M), [(W4, grid, 256, 2 * kStageBytes, 0, ALL)]
    return (Ho, Wo, K, M), [(W8, grid, 512, 2 * kStageBytes, 0, ALL)]


# ---------------------------------------------------------------------------------------------------------------------------
def draw(rng):
    """One random call: (mode, dynamic, shape..., flags).  Two in five are fp16x2 calls (that mode has four kinds of launch), a
    quarter of those candidates for the first-layer kernel (C_in = 4, whole tiles, no residual: a uniform draw hardly finds
    them); about one call in ten is one some mode rejects."""
    mode = ("bf16", "fp32", "fp32dyn", "fp16x2", "fp16x2")[int(rng.integers(5))]
    B, H = int(rng.integers(1, 257)), int(rng.integers(7, 225))
    W = H if rng.integers(4) else int(rng.integers(7, 225))
    Cin = (4, 64, 128, 384)[int(rng.integers(4))]
    Cout = 128 * int(rng.integers(1, 5)) if rng.integers(2) else 8 * int(rng.integers(1, 129))          # whole tiles / ragged
    k, s, p = ((4, 2, 1), (3, 1, 1), (1, 1, 0))[int(rng.integers(3))]
    add, out_f32, out_padded = bool(rng.integers(2)), False, True
    if Cin == 4 and rng.integers(8):
        k, s, p = 4, 2, 1                                                       # (3 x 3 or 1 x 1 on 4 channels: rejected)
    if mode == "fp16x2":
        out_f32 = bool(rng.integers(2))
        out_padded = not out_f32 if rng.integers(16) else out_f32              # (fp32 and padded: rejected)
        if not rng.integers(4):
            B, H, Cin, Cout, add, out_f32, out_padded = 8 * cdiv(B, 8), 16 * cdiv(H, 16), 4, 128 * int(rng.integers(1, 5)), False, False, True
            W, (k, s, p) = H, (4, 2, 1)
    else:
        out_padded = bool(rng.integers(4))
    if mode.startswith("fp32") and not rng.integers(3):                         # the shapes only the fp32 kernels take
        k, s, p = int(rng.integers(0, 6)), int(rng.integers(0, 3)), int(rng.integers(-1, 3))
        Cin = (4, 8, 12, 32, 64, 100)[int(rng.integers(6))]
    pick = int(rng.integers(40))
    if pick == 0:
        Cout += 4                                                               # a multiple of 4, not of 8
    elif pick == 1:
        Cout += 2
    elif pick == 2:
        B = 0
    elif pick == 3:
        H = (0, -3, 1, 2)[int(rng.integers(4))]
    elif pick == 4:
        Cin = (96, 32, 0, 6)[int(rng.integers(4))]
    return mode, B, H, W, Cin, Cout, k, s, p, add, out_f32, out_padded


def parent(mode, B, H, W, Cin, Cout, k, s, p, add, out_f32, out_padded, conv_waves, cus):
    if mode == "bf16":
        return parent_bf16(B, H, W, Cin, Cout, k, s, p, add, out_padded)
    if mode == "fp16x2":
        return parent_f16x2(B, H, W, Cin, Cout, k, s, p, add, out_padded, out_f32, conv_waves, cus)
    return parent_f32(B, H, W, Cin, Cout, k, s, p, add, out_padded, mode == "fp32dyn")


def kind(want):
    """The launch kind of a transcribed plan: the kernel, "dyn" for the fp32 pair, None for a rejected or empty call."""
    if want is None or not want[1]:
        return None if want is None else "empty"
    return "dyn" if len(want[1]) == 2 else want[1][0][0]


def sweep(ops, waves, cases, seed):
    from mem_amd import _lib
    rng = np.random.default_rng(seed)
    seen = Counter()
    for conv_waves in (4, 8, 16, 32):
        waves(conv_waves)
        for _ in range(cases):
            call = draw(rng)
            cus = (64, 128, 256, 304)[int(rng.integers(4))]
            want = parent(*call, conv_waves, cus)
            mode, B, H, W, Cin, Cout, k, s, p, add, out_f32, out_padded = call
            args = (mode.replace("dyn", ""), B, H, W, Cin, Cout, k, s, p)
            kw = dict(add=add, out_f32=out_f32, out_padded=out_padded, dynamic=mode == "fp32dyn", device_cus=cus)
            seen[kind(want)] += 1
            if want is None:
                with pytest.raises(_lib.MemhipError, match=r"failed \(-1\)"):      # MEMHIP_EINVAL, as from the call
                    ops.conv_plan(*args, **kw)
                continue
            got = ops.conv_plan(*args, **kw)
            assert ((got.Ho, got.Wo, got.K, got.M), got.launches) == want, (call, conv_waves, cus, got.launches, want)
            if want[1]:
                assert (got.Hp, got.Wp, got.off) == (H + 2, W + 2, 1 - p), call
            # never an empty grid, never more LDS than a workgroup can have
            for _, grid, block, lds, lo, hi in got.launches:
                assert grid >= 1 and block in (256, 512) and 0 < lds <= KMAX and 0 <= lo < hi <= ALL, (call, got.launches)
    return seen


def test_plan_equals_the_parent_cascades(ops, waves):
    """24 000 random calls (modes bf16 / fp32 static / fp32 dynamic / fp16x2, conv_waves 4 / 8 / 16 / 32, 64 / 128 / 256 / 304
    CUs, C_in 4 / 64 / 128 / 384, C_out in whole and ragged 128-tiles, H 7..224, B 1..256, residual and fp32 output on / off, and
    calls the launchers reject): geometry and ordered launches equal what the launchers of a9a608d computed, rejected calls are
    rejected with MEMHIP_EINVAL."""
    seen = sweep(ops, waves, 6000, 20261018)
    total = sum(seen.values())
    assert total == 24000
    # the sweep is not vacuous: every kind of launch (counted on the transcription alone) is at least 2 % of it, and so are
    # the rejected calls
    for k in (BF16, F32, "dyn", W4, W8, WIDE, FIRST, None):
        assert seen[k] >= 0.02 * total, (k, seen)
    assert seen["empty"] >= 100


def base_layers():
    """(H, C_in, C_out, k, s, p, residual, head) of the BASE tokenizer's 14 convolutions: 224^2, four strided layers to 14 x 14,
    hidden 384, three ResBlocks, 8192 tokens."""
    L, h, cin = [], 224, 4
    for _ in range(4):
        L.append((h, cin, 384, 4, 2, 1, False, False))
        h, cin = h // 2, 384
    for _ in range(3):
        L += [(h, 384, 384, 3, 1, 1, False, False), (h, 384, 384, 3, 1, 1, False, False), (h, 384, 384, 1, 1, 0, True, False)]
    return L + [(h, 384, 8192, 1, 1, 0, False, True)]


def test_worked_numbers(ops, waves):
    """256 CUs, default options (conv_waves = 16), the BASE tokenizer."""
    def plans(B):
        return [ops.conv_plan("fp16x2", B, h, h, ci, co, k, s, p, add=add, out_f32=head, out_padded=not head, device_cus=256)
                for h, ci, co, k, s, p, add, head in base_layers()]
    P = plans(256)
    # the first layer: persistent, 256 // 3 workgroups per column tile of the weights
    assert P[0].launches == [(FIRST, 255, 512, 135168, 0, ALL)] and (P[0].Ho, P[0].K, P[0].M) == (112, 64, 256 * 112 * 112)
    # every other layer: the wide tile; the 14 x 14, 384-channel layers at 588 workgroups = 2.3 rounds of the chip
    assert all(p.launches[0][0] == WIDE for p in P[1:])
    assert all(p.launches == [(WIDE, 588, 512, 147456, 0, ALL)] for p in P[4:13])
    assert P[13].launches[0][1] == 196 * 64 and [p.launches[0][1] for p in P[1:4]] == [3136 * 3, 784 * 3, 196 * 3]
    # batch 2: the 14 x 14 layers fall back to eight waves on 128 x 128 tiles; the first layer stays persistent (whole tiles)
    P = plans(2)
    assert all(p.launches == [(W8, 4 * 3, 512, 131072, 0, ALL)] for p in P[4:13])
    assert P[0].launches == [(FIRST, 255, 512, 135168, 0, ALL)]
    # the fp32 dynamic pair: the 32-row form below the switch point, the 128-row form from it on
    p = ops.conv_plan("fp32", 256, 56, 56, 384, 384, 3, 1, 1, dynamic=True, device_cus=256)
    assert p.launches == [(F32M32, 2048, 256, 43520, 0, 7), (F32, 1024, 256, 69632, 7, ALL)]
    p = ops.conv_plan("fp32", 256, 14, 14, 384, 384, 3, 1, 1, dynamic=True, device_cus=256)
    assert p.launches == [(F32M32, 2048, 256, 43520, 0, 112), (F32, 1024, 256, 69632, 112, ALL)]
    p = ops.conv_plan("fp32", 3, 14, 14, 64, 256, 1, 1, 0, dynamic=True, device_cus=256)
    assert [l[1:3] for l in p.launches] == [(19 * 2, 256), (5 * 2, 256)] and p.launches[0][5] == p.launches[1][4] == 168
    # static fp32 and bf16: one 128 x 128 tile per workgroup
    assert ops.conv_plan("fp32", 256, 14, 14, 384, 384, 3, 1, 1, device_cus=256).launches == [(F32, 392 * 3, 256, 69632, 0, ALL)]
    assert ops.conv_plan("bf16", 256, 14, 14, 384, 384, 3, 1, 1, device_cus=256).launches == [(BF16, 392 * 3, 256, 65536, 0, ALL)]
    # the other option values
    waves(8)
    assert plans(256)[0].launches[0][:3] == (W8, 25088 * 3, 512) and plans(256)[5].launches[0][:2] == (W8, 392 * 3)
    waves(4)
    assert plans(256)[5].launches == [(W4, 392 * 3, 256, 131072, 0, ALL)]
    waves(32)
    assert plans(2)[5].launches[0][:2] == (WIDE, 2 * 3) and plans(2)[0].launches[0][0] == FIRST
    assert ops.conv_plan("fp16x2", 0, 14, 14, 384, 384, 3, 1, 1, device_cus=256).launches == []


def test_query_validates_like_the_call(ops):
    """Per mode, with the launcher's own message."""
    from mem_amd import _lib
    for mode, name in (("bf16", "conv2d"), ("fp16x2", "conv2d_f16x2")):
        with pytest.raises(_lib.MemhipError, match=name + ": only the encoder's shapes"):
            ops.conv_plan(mode, 2, 14, 14, 64, 64, 2, 2, 0, device_cus=256)
        with pytest.raises(_lib.MemhipError, match=name + ": C_in must be 4 \\(first layer, 4x4\\) or a multiple of 64"):
            ops.conv_plan(mode, 2, 14, 14, 32, 64, 3, 1, 1, device_cus=256)
        with pytest.raises(_lib.MemhipError, match=name + ": C_out must be a multiple of 8"):
            ops.conv_plan(mode, 2, 14, 14, 64, 36, 3, 1, 1, device_cus=256)
        with pytest.raises(_lib.MemhipError, match=name + ": bad shape"):
            ops.conv_plan(mode, -1, 14, 14, 64, 64, 3, 1, 1, device_cus=256)
    with pytest.raises(_lib.MemhipError, match="conv2d_f16x2: the fp32 output is the dense token-logit matrix"):
        ops.conv_plan("fp16x2", 2, 14, 14, 64, 64, 3, 1, 1, out_f32=True, out_padded=True, device_cus=256)
    # the fp32 kernels take what the others do not -- and alone can be asked for an empty output
    assert ops.conv_plan("fp32", 3, 10, 10, 8, 12, 2, 2, 0, device_cus=256).launches == [(F32, 1, 256, 69632, 0, ALL)]
    with pytest.raises(_lib.MemhipError, match="conv2d_f32: empty output"):
        ops.conv_plan("fp32", 3, 2, 2, 8, 12, 4, 1, 0, device_cus=256)
    with pytest.raises(_lib.MemhipError, match="conv2d_f32: K = 36 must be a multiple of 32"):
        ops.conv_plan("fp32", 3, 14, 14, 4, 12, 3, 1, 1, device_cus=256)
    with pytest.raises(_lib.MemhipError, match="conv2d_f32: kernel size 1..4"):
        ops.conv_plan("fp32", 3, 14, 14, 8, 12, 5, 1, 1, device_cus=256)
    with pytest.raises(_lib.MemhipError, match="conv2d_f32: C_in and C_out must be multiples of 4"):
        ops.conv_plan("fp32", 3, 14, 14, 8, 10, 2, 1, 1, device_cus=256)
