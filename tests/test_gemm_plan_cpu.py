"""-m "not gpu": the dispatch table of memhip_gemm_bf16_nt, checked through the plan query
memhip_gemm_bf16_nt_plan.  The query validates and plans like the GEMM itself and launches nothing: pointers are placeholders
that are never read."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

(BIAS_BF16, BIAS_GELU, RESIDUAL, DGELU, F32, PATCH_EMBED, BIAS_GELU_DG, MUL_AUX, RESIDUAL_DROP) = range(9)
NT128, G256, P8_256, P8_128, P8_PAIR = range(5)
PAIRED = (BIAS_BF16, RESIDUAL, BIAS_GELU_DG, MUL_AUX)
PTR = 0x10000          # any 16-byte aligned non-null address

# the option settings of tools/resid_gemm_probe.py and tools/rem_probe.py
SETTINGS = ({}, {"gemm_p8_pair": 0}, {"gemm_p8_half": 0}, {"gemm_p8": 0}, {"gemm_p8": 0, "gemm256": 0}, {"gemm_split": 0})


@pytest.fixture(scope="module")
def ops():
    from mem_amd import ops
    return ops


def make_args(ops, M, N, K, epi, out0=True, rowmask=False, sample_map=False, rps=197, ld_odd=False):
    """Valid arguments of epilogue `epi`; every leading dimension N (a multiple of 8) unless ld_odd.  Returns (args, keepalive)."""
    a = ops.GemmArgs()
    a.A = a.B = PTR
    a.lda = a.ldb = K
    a.M, a.N, a.K, a.epilogue = M, N, K, epi
    a.keep_prob, a.colscale, a.rows_per_sample = 1.0, 1.0, 1
    drop = None
    if epi in (BIAS_BF16, BIAS_GELU, DGELU, F32, BIAS_GELU_DG, MUL_AUX) or (epi == RESIDUAL and out0):
        a.out0, a.ldo0 = PTR, N + (4 if ld_odd else 0)
    if epi in (BIAS_GELU, BIAS_GELU_DG):
        a.out1, a.ldo1 = PTR, N
    if epi in (DGELU, MUL_AUX):
        a.aux, a.ldaux = PTR, N
    if epi in (RESIDUAL, RESIDUAL_DROP):
        a.resid, a.ldr, a.rows_per_sample, a.keep_prob = PTR, N + (4 if ld_odd and not a.out0 else 0), rps, 0.9
        if rowmask:
            a.rowmask = PTR
        elif sample_map:
            a.sample_map = PTR
    if epi == RESIDUAL_DROP:
        drop = ops.dropout_params(1, 2, 3, 0.1)
        a.dropout = C.addressof(drop)
    if epi == PATCH_EMBED:
        a.resid, a.ldr, a.vec1, a.aux, a.rows_per_sample = PTR, N, PTR, PTR, 196
    return a, drop


def plan(ops, a, stream_cus, device_cus):
    return [(l.kind, l.row0, l.rows, l.tail_rows, bool(l.guard), bool(l.copy), l.grid, l.tail_grid)
            for l in ops.gemm_nt_plan(a[0], stream_cus, device_cus)]


def kinds(p):
    return [(l[0], l[2]) for l in p]


def cdiv(a, b):
    return -(-a // b)


def test_worked_cases(ops):
    """DESIGN.md section 4 at 256 CUs, default options, leading dimensions multiples of 8."""
    def k(M, N, K, epi, cus=256, dev=256, **kw):
        return kinds(plan(ops, make_args(ops, M, N, K, epi, **kw), cus, dev))
    # (50432, 768, 768): 591 tiles = 2 rounds + 79 (at most half of 256): head (2 * 256 / 3) * 256 = 43520, tail 6912
    S = (50432, 768, 768)
    for epi in PAIRED:
        p = plan(ops, make_args(ops, *S, epi, out0=False), 256, 256)
        assert p == [(P8_PAIR, 0, 43520, 6912, False, epi != RESIDUAL, 256, 162)], (epi, p)
    for epi in (F32, BIAS_GELU, DGELU):
        assert k(*S, epi) == [(P8_256, 43520), (P8_128, 6912)], epi
    assert k(*S, RESIDUAL_DROP) == [(P8_128, 43520), (P8_128, 6912)]
    assert k(*S, RESIDUAL, out0=True) == [(P8_128, 43520), (P8_128, 6912)]
    # remainder 237 of 256: more than half, no split
    assert k(50432, 2304, 768, BIAS_BF16) == [(P8_256, 50432)]
    # less than one round, M no multiple of 256; the tail is below 128 rows: no pair, no 128-row p8
    for epi in (BIAS_BF16, F32, RESIDUAL):
        assert k(4196, 768, 768, epi, out0=False) == [(P8_256, 4096), (NT128, 100)], epi
    assert k(4196, 768, 768, RESIDUAL_DROP) == [(P8_128, 4096), (NT128, 100)]
    assert k(4095, 1024, 192, F32) == [(NT128, 4095)]
    assert k(8193, 768, 64, F32) == [(NT128, 8193)]
    p = plan(ops, make_args(ops, 4097, 3072, 320, F32), 256, 256)
    assert p == [(G256, 0, 4097, 0, False, False, min(17 * 12, 256), 0)], p
    assert k(4097, 3072, 320, MUL_AUX) == [(NT128, 4097)]              # not one of gemm256's six epilogues
    assert k(50432, 768, 512, PATCH_EMBED) == [(NT128, 50432)]         # never split
    # 252 CUs (no multiple of 8): no pair; 2 rounds + 87: head (2 * 252 / 3) * 256 = 43008
    assert k(*S, BIAS_BF16, cus=252) == [(P8_256, 43008), (P8_128, 7424)]
    # no CUs for the stream: no p8 form, and N is below gemm256's 1024
    assert k(*S, BIAS_BF16, cus=0) == [(NT128, 50432)]
    assert k(50432, 2304, 768, BIAS_BF16, cus=0, dev=248) == [(G256, 50432)]
    assert k(50432, 2304, 768, BIAS_BF16, cus=0, dev=0) == [(NT128, 50432)]
    # a head that no p8 form takes (248 CUs, 16 tiles wide: 272 tiles = 1 round + 24, head (248 / 16) * 256 = 3840 rows, below
    # 4096) sends the WHOLE product on
    assert k(4352, 4096, 128, BIAS_BF16, cus=248) == [(G256, 4352)]
    assert k(4352, 4096, 128, MUL_AUX, cus=248) == [(NT128, 4352)]
    assert k(4352, 4096, 128, MUL_AUX, cus=256) == [(P8_PAIR, 4096)]
    # the split and pair decisions look at the row counts: a sample map needs rows below 2^21 and rows_per_sample >= 86
    assert k(*S, RESIDUAL, out0=False, sample_map=True, rps=197) == [(P8_PAIR, 43520)]
    assert k(*S, RESIDUAL, out0=False, sample_map=True, rps=17) == [(NT128, 50432)]
    assert k(0, 768, 768, F32) == []


def test_query_validates_like_the_gemm(ops):
    from mem_amd import _lib
    a, _ = make_args(ops, 4096, 768, 768, BIAS_BF16)
    a.out0 = None
    with pytest.raises(_lib.MemhipError, match="out0"):
        ops.gemm_nt_plan(a, 256, 256)
    a, _ = make_args(ops, 4096, 768, 96, F32)
    with pytest.raises(_lib.MemhipError, match="multiple of 64"):
        ops.gemm_nt_plan(a, 256, 256)


def test_plan_properties_over_a_sweep(ops):
    """Seeded sweep: M in [1, 60000], N = 8 * [1, 520], K = 64 * [1, 48], all nine epilogues with and without out0 / rowmask /
    sample_map (17 and 197 rows per sample), CU counts {256, 248, 240, 64, 8, 0}, the probe tools' option settings."""
    from mem_amd import _lib
    rng = np.random.default_rng(20240)
    CUS = (256, 248, 240, 64, 8, 0)
    seen, combos = Counter(), Counter()
    try:
        for opts in SETTINGS:
            for name, v in opts.items():
                _lib.set_option(name, v)
            for _ in range(12000):
                M = int(rng.integers(1, 60001))
                # (every 4th N a multiple of 256, every 2nd K of 128: the shapes the persistent forms take at all)
                N = 256 * int(rng.integers(1, 17)) if rng.integers(4) == 0 else 8 * int(rng.integers(1, 521))
                K = 64 * int(rng.integers(1, 49))
                epi = int(rng.integers(9))
                out0, per_sample, rps = bool(rng.integers(2)), int(rng.integers(3)), (17, 197)[int(rng.integers(2))]
                ld_odd = rng.integers(16) == 0
                cus, dev = CUS[int(rng.integers(6))], CUS[int(rng.integers(6))]
                a = make_args(ops, M, N, K, epi, out0=out0, rowmask=per_sample == 1, sample_map=per_sample == 2, rps=rps,
                              ld_odd=ld_odd)
                p = plan(ops, a, cus, dev)
                ctx = (opts, M, N, K, epi, out0, per_sample, rps, ld_odd, cus, dev, p)
                ntn = N // 256
                # the launches cover [0, M) exactly once, in row order
                row = 0
                for kind, row0, rows, tail, guard, copy, grid, tail_grid in p:
                    assert row0 == row and rows > 0, ctx
                    row += rows + tail
                    assert tail == 0 or kind == P8_PAIR, ctx
                    if kind != NT128:
                        vec = all(ld % 8 == 0 for ld in (a[0].ldo0, a[0].ldo1, a[0].ldr, a[0].ldaux))
                        assert N % 256 == 0 and vec and K % (64 if kind == G256 else 128) == 0, ctx
                    if kind in (P8_256, P8_128, P8_PAIR):
                        assert opts.get("gemm_p8", 1) and cus > 0 and epi != PATCH_EMBED, ctx
                        assert not (a[0].sample_map and rps < 86), ctx
                        assert copy == (not (epi == RESIDUAL_DROP or (epi == RESIDUAL and not a[0].out0))), ctx
                    if kind in (P8_256, P8_PAIR):
                        assert rows % 256 == 0 and epi != RESIDUAL_DROP and not (epi == RESIDUAL and a[0].out0), ctx
                        assert grid == min(rows // 256 * ntn, cus), ctx
                    if kind == P8_256:
                        assert not guard and tail_grid == 0, ctx
                    if kind == P8_128:
                        assert guard == (rows % 128 != 0) and grid == min(cdiv(rows, 128) * ntn, cus) and tail_grid == 0, ctx
                    if kind == P8_PAIR:
                        assert epi in PAIRED and tail >= 128 and cus % 8 == 0, ctx
                        assert opts.get("gemm_p8_pair", 1) and opts.get("gemm_p8_half", 1), ctx
                        assert guard == (tail % 128 != 0) and tail_grid == min(cdiv(tail, 128) * ntn, cus), ctx
                    if kind == G256:
                        assert opts.get("gemm256", 1) and dev > 0 and len(p) == 1, ctx
                        assert not guard and not copy and grid == min(cdiv(M, 256) * ntn, dev) and tail_grid == 0, ctx
                    if kind == NT128:
                        assert not guard and not copy and grid == cdiv(rows, 128) * cdiv(N, 128) and tail_grid == 0, ctx
                assert row == M, ctx
                assert len(p) == 1 or p[0][0] in (P8_256, P8_128), ctx          # only a p8 head is followed by a second launch
                assert len(p) == 1 or opts.get("gemm_split", 1), ctx
                for l in p:
                    seen[l[0]] += 1
                if len(p) == 2:
                    combos[(p[0][0], p[1][0])] += 1
            for name in opts:
                _lib.set_option(name, 1)
    finally:
        for name in ("gemm_p8", "gemm256", "gemm_split", "gemm_p8_half", "gemm_p8_pair"):
            _lib.set_option(name, 1)
    # the sweep is not vacuous
    for kind in (NT128, G256, P8_256, P8_128, P8_PAIR):
        assert seen[kind] >= 20, (kind, seen)
    for combo in ((P8_256, P8_128), (P8_128, P8_128), (P8_256, NT128), (P8_128, NT128)):
        assert combos[combo] >= 20, (combo, combos)
    assert set(combos) == {(P8_256, P8_128), (P8_128, P8_128), (P8_256, NT128), (P8_128, NT128)}, combos
