"""-m "not gpu": the dispatch of the weight-gradient GEMMs (memhip_gemm_bf16_tn / _tn_group), checked through the
plan query memhip_gemm_bf16_tn_plan against a transcription of the launchers the plan replaced (group dispatch -> single
dispatch -> the 128 x 128 kernel's inline arithmetic), and the two workspace queries against a transcription of theirs.
The query validates and plans like the calls and launches nothing: pointers are placeholders of which only the address
bits are read."""
import random
from collections import Counter

import pytest

T128, ATOMIC, WS, GROUP = range(4)
PTR = 0x10000            # any 16-byte aligned non-null address
WIDTHS = (256, 512, 768, 1024, 2304, 3072)
AMPLE = 1 << 40


@pytest.fixture(scope="module")
def ops():
    from mem_amd import ops
    return ops


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- the parent's launchers, transcribed
# a problem is (R, N, K, out address, ldo); a launch is
# (kind, grid, reduce_grid, memset_first, use_atomics, ws_bytes, ((problem, tiles, splits, rows_per_split, wg_begin, quad_begin, ws_offset), ...))

def old_p8_plan(R, N, K, num_cu):
    tiles = (N // 256) * (K // 256)
    pairs = cdiv(R, 128)
    splits = num_cu // tiles
    if splits < 1:
        splits = 1
    if splits > pairs // 2:
        splits = pairs // 2 if pairs // 2 > 0 else 1
    rows = cdiv(pairs, splits) * 128
    return tiles, cdiv(R, rows), rows


def old_group_plan(pr, num_cu):
    """None, "shape" or "slices" when tn_group_plan says no; else (parts, workgroups, quads, workspace floats)"""
    if len(pr) < 2 or len(pr) > 4 or not num_cu:
        return "shape"
    tiles_total = 0
    for R, N, K, out, ldo in pr:
        if N % 256 != 0 or K % 256 != 0 or R < 2048 or ldo % 4 != 0 or out & 15:
            return "shape"
        tiles_total += (N // 256) * (K // 256)
    best_s, best_eff = 0, 0.0
    for r in range(1, 5):
        sp = (r * num_cu) // tiles_total
        if sp < 2:
            continue
        eff = float(tiles_total) * sp / (float(r) * num_cu)
        if eff > best_eff + 1e-9:
            best_eff, best_s = eff, sp
        if eff >= 0.80:
            break
    if best_s < 2:
        return "slices"
    wgs = quads = floats = 0
    parts = []
    for i, (R, N, K, out, ldo) in enumerate(pr):
        tiles = (N // 256) * (K // 256)
        pairs = cdiv(R, 128)
        sp = best_s
        if sp > pairs // 2:
            sp = pairs // 2 if pairs // 2 > 0 else 1
        rows = cdiv(pairs, sp) * 128
        splits = cdiv(R, rows)
        parts.append((i, tiles, splits, rows, wgs, quads, floats))
        wgs += tiles * splits
        quads += (N * K // 4 + 255) // 256 * 256
        floats += splits * N * K
    return tuple(parts), wgs, quads, floats


def old_single(i, q, accumulate, ws, ws_bytes, num_cu, p8_on):
    """memhip_gemm_bf16_tn behind its validation (R > 0)"""
    R, N, K, out, ldo = q
    if p8_on and N % 256 == 0 and K % 256 == 0 and R >= 2048 and num_cu:           # gemm_tn_p8_dispatch
        tiles, splits, rows = old_p8_plan(R, N, K, num_cu)
        need = splits * N * K * 4
        part = ((i, tiles, splits, rows, 0, 0, 0),)
        if ws and splits > 1 and ws_bytes >= need and ws & 15 == 0 and ldo % 4 == 0 and out & 15 == 0:
            return (WS, tiles * splits, (N * K // 4 + 255) // 256, 0, 0, need, part)
        return (ATOMIC, tiles * splits, 0, int(not accumulate), 1, 0, part)
    tiles = cdiv(N, 128) * cdiv(K, 128)
    stages = cdiv(R, 64)
    splits = cdiv(768, tiles)
    if splits > stages // 4:
        splits = stages // 4
    if splits < 1:
        splits = 1
    rows = cdiv(stages, splits) * 64
    splits = cdiv(R, rows)
    return (T128, tiles * splits, 0, int(splits > 1 and not accumulate), int(splits > 1 or bool(accumulate)), 0,
            ((i, tiles, splits, rows, 0, 0, 0),))


def old_group_call(pr, accumulate, ws, ws_bytes, num_cu, p8_on, group_on):
    """memhip_gemm_bf16_tn_group behind its validation: (launches, why a wanted group was declined or None)"""
    why = None
    if all(q[0] > 0 for q in pr) and len(pr) > 1 and p8_on and group_on:
        if ws and ws & 15 == 0:                                                     # gemm_tn_p8_group_dispatch
            g = old_group_plan(pr, num_cu)
            if not isinstance(g, str):
                parts, wgs, quads, floats = g
                if floats * 4 <= ws_bytes:
                    return [(GROUP, wgs, quads // 256, 0, 0, floats * 4, parts)], None
                why = "bytes"
            else:
                why = g
        else:
            why = "workspace"
    return [old_single(i, q, accumulate, ws, ws_bytes, num_cu, p8_on) for i, q in enumerate(pr) if q[0] > 0], why


def old_workspace(R, N, K, device_cus):
    if N % 256 != 0 or K % 256 != 0 or R < 2048 or not device_cus:
        return 0
    need = 0
    for cu in range(device_cus, 7, -8):
        _, splits, _ = old_p8_plan(R, N, K, cu)
        need = max(need, splits * N * K * 4 if splits > 1 else 0)
    return need


def old_group_workspace(pr, device_cus):
    need = 0
    for cu in range(device_cus, 7, -8):
        g = old_group_plan(pr, cu)
        if not isinstance(g, str):
            need = max(need, g[3] * 4)
    return max([need] + [old_workspace(R, N, K, device_cus) for R, N, K, _, _ in pr])


# ---------------------------------------------------------------- the library's plan
def problems(ops, pr):
    arr = (ops.TnProblem * len(pr))()
    for q, (R, N, K, out, ldo) in zip(arr, pr):
        q.A, q.B, q.lda, q.ldb, q.out, q.ldo, q.R, q.N, q.K = PTR, PTR, N, K, out, ldo, R, N, K
    return arr


def new_plan(ops, pr, accumulate, ws, ws_bytes, cus):
    return [(l.kind, l.grid, l.reduce_grid, l.memset_first, l.use_atomics, l.ws_bytes,
             tuple((p.problem, p.tiles, p.splits, p.rows_per_split, p.wg_begin, p.quad_begin, p.ws_offset)
                   for p in l.p[:l.count]))
            for l in ops.gemm_tn_plan(problems(ops, pr), accumulate, (ws, ws_bytes), cus)]


def dense(shapes):
    return [(R, N, K, PTR, K) for R, N, K in shapes]


def test_worked_numbers(ops):
    """256 CUs, default options, an ample workspace; singles as (tiles, slices, rows per slice)"""
    def single(shape, cus=256, accumulate=True, ws=PTR):
        (l,) = new_plan(ops, dense([shape]), accumulate, ws, AMPLE if ws else 0, cus)
        return l
    for shape, want in (((50432, 768, 768), (9, 27, 1920)), ((50432, 2304, 768), (27, 9, 5632)),
                        ((50432, 3072, 768), (36, 7, 7296)), ((2048, 256, 256), (1, 8, 256))):
        l = single(shape)
        assert l[0] == WS and l[6][0][1:4] == want and l[1] == want[0] * want[1], (shape, l)
        assert l[5] == want[1] * shape[1] * shape[2] * 4 and l[2] == shape[1] * shape[2] // 1024
        assert single(shape, ws=None)[0] == ATOMIC
    assert single((2048, 256, 256), cus=8)[6][0][1:4] == (1, 8, 256)
    # groups: one grid, one common slice count
    M = 50432
    (g,) = new_plan(ops, dense([(M, 768, 768), (M, 2304, 768)]), False, PTR, AMPLE, 256)          # proj + qkv: common 7
    assert g[:5] == (GROUP, 63 + 189, (768 * 768 + 2304 * 768) // 1024, 0, 0)
    assert g[6] == ((0, 9, 7, 7296, 0, 0, 0), (1, 27, 7, 7296, 63, 768 * 768 // 4, 7 * 768 * 768))
    assert g[5] == 7 * (768 * 768 + 2304 * 768) * 4
    (g,) = new_plan(ops, dense([(M, 768, 3072), (M, 3072, 768)]), False, PTR, AMPLE, 256)         # fc2 + fc1: common 3
    assert g[0] == GROUP and g[1] == 216 and [p[1:4] for p in g[6]] == [(36, 3, 16896)] * 2
    # the 128 x 128 kernel: one slice that overwrites uses plain stores and no memset
    assert single((70, 768, 512), accumulate=False) == (T128, 24, 0, 0, 0, 0, ((0, 24, 1, 128, 0, 0, 0),))
    assert single((70, 768, 512), accumulate=True)[3:5] == (0, 1)
    assert single((1200, 768, 768), accumulate=False) == (T128, 36 * 4, 0, 1, 1, 0, ((0, 36, 4, 320, 0, 0, 0),))
    # the p8 atomic form clears `out` whenever it overwrites, even with one slice (16 tiles on 8 CUs)
    assert single((2048, 1024, 1024), cus=8, accumulate=False)[:5] == (ATOMIC, 16, 0, 1, 1)
    # R == 0: no launch, whatever the neighbours do
    p = new_plan(ops, dense([(0, 768, 768), (M, 768, 768)]), False, PTR, AMPLE, 256)
    assert [l[0] for l in p] == [WS] and p[0][6][0][0] == 1
    assert new_plan(ops, dense([(0, 768, 768)]), False, PTR, AMPLE, 256) == []


def test_query_validates_like_the_group_call(ops):
    from mem_amd import _lib
    with pytest.raises(_lib.MemhipError, match=r"1\.\.4 problems, got 5"):
        ops.gemm_tn_plan(problems(ops, dense([(2048, 256, 256)] * 5)), True, None, 256)
    with pytest.raises(_lib.MemhipError, match=r"gemm_tn_group\[1\]: bad shape"):
        ops.gemm_tn_plan(problems(ops, dense([(2048, 256, 256), (-1, 256, 256)])), True, None, 256)
    arr = problems(ops, dense([(2048, 256, 256)]))
    arr[0].out = None
    with pytest.raises(_lib.MemhipError, match="null pointer"):
        ops.gemm_tn_plan(arr, True, None, 256)
    with pytest.raises(_lib.MemhipError, match="16-byte aligned"):
        ops.gemm_tn_plan(problems(ops, dense([(2048, 260, 256)])), True, None, 256)


def random_call(rng):
    """(problems, accumulate, ws, ws_bytes, cus, tn_p8, tn_group)"""
    count = rng.choice((1, 2, 2, 3, 4))
    cus = 8 * rng.randint(1, 32)
    p8_on, group_on = int(rng.random() < 0.85), int(rng.random() < 0.85)
    friendly = rng.random() < 0.5
    shared = rng.randint(2048, 60000)
    pr = []
    for _ in range(count):
        if friendly:
            R = shared if rng.random() < 0.7 else rng.randint(2048, 60000)
            N, K = rng.choice(WIDTHS), rng.choice(WIDTHS)
        else:
            R = rng.choice((0, rng.randint(1, 4096), rng.randint(1, 60000)))
            N, K = (rng.choice(WIDTHS) if rng.random() < 0.5 else 8 * rng.randint(1, 400) for _ in range(2))
        out, ldo = PTR, K
        if rng.random() < (0.05 if friendly else 0.20):        # a view the reduction passes cannot take
            if rng.random() < 0.5:
                out += 4
            else:
                ldo += 2
        pr.append((R, N, K, out, ldo))
    small = pr[0][1] * pr[0][2] * 4                            # one slab of the first product
    ws_bytes = rng.choice((AMPLE, AMPLE, AMPLE, small, 0) if friendly else (0, small, AMPLE))
    ws = (PTR + (8 if rng.random() < 0.04 else 0)) if ws_bytes else 0
    return pr, rng.randint(0, 1), ws, ws_bytes, cus, p8_on, group_on


def test_plan_equals_the_launchers_it_replaced(ops):
    """24 000 seeded calls: the plan equals the transcription field by field, both workspace queries equal theirs (the
    single one is the group one of a lone dense product), and every outcome is a fair share of the calls."""
    from mem_amd import _lib
    rng = random.Random(20261)
    seen = Counter()
    calls = 24000
    try:
        for _ in range(calls):
            pr, accumulate, ws, ws_bytes, cus, p8_on, group_on = random_call(rng)
            _lib.set_option("tn_p8", p8_on)
            _lib.set_option("tn_group", group_on)
            ctx = (pr, accumulate, hex(ws), ws_bytes, cus, p8_on, group_on)
            want, why = old_group_call(pr, accumulate, ws, ws_bytes, cus, p8_on, group_on)
            got = new_plan(ops, pr, accumulate, ws or None, ws_bytes, cus)
            assert got == want, (ctx, got, want)
            # the workspace queries read neither the options nor the caller's workspace
            assert ops.gemm_tn_plan_workspace(problems(ops, pr), cus) == old_group_workspace(pr, cus), ctx
            R, N, K = pr[0][:3]
            assert ops.gemm_tn_plan_workspace(problems(ops, dense([(R, N, K)])), cus) == old_workspace(R, N, K, cus), ctx
            outcomes = set()
            for l in want:
                outcomes.add({GROUP: "group", WS: "p8_ws", ATOMIC: "p8_atomic"}.get(l[0]) or
                             ("128_split" if l[6][0][2] > 1 else "128_one"))
            if any(q[0] == 0 for q in pr):
                outcomes.add("r0")
            if why == "slices":
                outcomes.add("declined_by_slices")
            seen.update(outcomes)
    finally:
        _lib.set_option("tn_p8", 1)
        _lib.set_option("tn_group", 1)
    print({k: round(v / calls, 4) for k, v in sorted(seen.items())})
    for outcome in ("group", "p8_ws", "p8_atomic", "128_split", "128_one", "r0"):
        assert seen[outcome] >= 0.02 * calls, (outcome, seen)
    assert seen["declined_by_slices"] >= 0.01 * calls, seen
