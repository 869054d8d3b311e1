"""-m "not gpu": the dispatch of memhip_attn_fwd / memhip_attn_bwd* (DESIGN.md section 4), checked through the plan queries
memhip_attn_plan_fwd / memhip_attn_plan_bwd.  The queries validate and plan like the calls themselves and launch nothing; the
workspace address is a placeholder that is never read."""
from collections import Counter

import numpy as np
import pytest

A16, SMALL, WIN, WIN_DS, STREAM = range(1, 6)
PTR = 0x10000          # any 16-byte aligned non-null address
KMAX = 160 * 1024      # LDS bytes a workgroup may use
CUS = (0, 8, 64, 248, 256, 304)
OPTIONS = [(a16, win) for a16 in (1, 0) for win in (1, 0, 2)]


@pytest.fixture(scope="module")
def ops():
    from mem_amd import ops
    return ops


@pytest.fixture
def options():
    """set(attn16, attn_win); the defaults (1, 1) come back afterwards."""
    from mem_amd import _lib

    def set_(attn16, attn_win):
        _lib.set_option("attn16", attn16)
        _lib.set_option("attn_win", attn_win)
    yield set_
    set_(1, 1)


def fam(ops, B, win, H=12, cus=256, **kw):
    return ops.attn_plan(B, win[0] * win[1] + 1, H, win, stream_cus=cus, **kw).family


def test_design_table_rows(ops, options):
    """The four attention rows of the DESIGN.md section 4 table, and the options that move a shape between them."""
    bwd = dict(backward=True)
    # row 1: 14 x 14, 197 tokens; backward without a v_bias gradient
    assert fam(ops, 256, (14, 14)) == A16 and fam(ops, 256, (14, 14), **bwd) == A16
    assert fam(ops, 256, (14, 14), out=True, **bwd) == A16 and fam(ops, 3, (14, 14), dtable=False, **bwd) == A16
    # row 2: up to 256 tokens otherwise; 14 x 14 with a v_bias gradient; a window 40 wide is not enough for the slot layout
    assert fam(ops, 256, (14, 14), dv_bias=True, **bwd) == SMALL
    for win in ((4, 4), (8, 8), (15, 17), (4, 9), (6, 40), (12, 20), (1, 255)):
        assert fam(ops, 5, win) == SMALL and fam(ops, 5, win, **bwd) == SMALL, win
    assert ops.attn_plan(5, 241, 3, (6, 40), stream_cus=256).n == 8
    # row 3: more than 256 tokens, window 40 or 20 wide; the dS-storing pair with a caller workspace
    for win in ((30, 40), (16, 20), (13, 20), (7, 40)):
        assert fam(ops, 4, win) == WIN and fam(ops, 4, win, **bwd) == WIN, win
        need = ops.attn_bwd_workspace(4, win[0] * win[1] + 1, 12, win)
        assert need > 0 and fam(ops, 4, win, ws=PTR, ws_bytes=need, **bwd) == WIN_DS, win
        assert fam(ops, 4, win, ws=PTR, ws_bytes=need - 1, **bwd) == WIN, win
        assert fam(ops, 4, win, ws=PTR + 8, ws_bytes=need, **bwd) == WIN, win           # not 16-byte aligned
        assert fam(ops, 4, win, ws=None, ws_bytes=need, **bwd) == WIN, win
    # row 4: more than 256 tokens, any other window
    for win in ((17, 19), (16, 16), (17, 17), (40, 30), (20, 16)):
        assert fam(ops, 4, win) == STREAM and fam(ops, 4, win, ws=PTR, ws_bytes=1 << 40, **bwd) == STREAM, win
        assert ops.attn_bwd_workspace(4, win[0] * win[1] + 1, 12, win) == 0
    # option attn16 = 0: the general kernels take 14 x 14
    options(0, 1)
    assert fam(ops, 256, (14, 14)) == SMALL and fam(ops, 256, (14, 14), **bwd) == SMALL
    assert fam(ops, 4, (30, 40)) == WIN
    # option attn_win = 0: the streaming kernels take the long windows; 2 (any non-zero value): the slot layout, but never the
    # dS-storing pair
    need = ops.attn_bwd_workspace(4, 1201, 12, (30, 40))
    options(1, 0)
    assert fam(ops, 4, (30, 40)) == STREAM and fam(ops, 4, (30, 40), ws=PTR, ws_bytes=need, **bwd) == STREAM
    assert fam(ops, 256, (14, 14)) == A16 and fam(ops, 4, (6, 40)) == SMALL
    options(1, 2)
    assert fam(ops, 4, (30, 40)) == WIN and fam(ops, 4, (30, 40), ws=PTR, ws_bytes=need, **bwd) == WIN
    assert fam(ops, 4, (16, 20), **bwd) == WIN


def test_worked_numbers(ops, options):
    """256 CUs, default options."""
    p = ops.attn_plan(256, 197, 12, (14, 14), stream_cus=256)
    assert (p.family, p.nwg, p.launches[0][1]) == (A16, 21, (252, 1, 1))
    p = ops.attn_plan(256, 197, 12, (14, 14), backward=True, out=True, stream_cus=256)
    assert (p.family, p.nwg, p.fd, p.launches) == (A16, 21, 1, [("attn16_bwd_kernel", (252, 1, 1), 448, 160016)])
    options(0, 1)
    for p in (ops.attn_plan(256, 197, 12, (14, 14), stream_cus=256), ops.attn_plan(256, 197, 12, (14, 14), backward=True, stream_cus=256)):
        assert (p.family, p.spb, p.n) == (SMALL, 13, 7) and all(l[1] == (240, 1, 1) for l in p.launches[-2:])
    options(1, 1)
    # 30 x 40 (ViT-L at 480 x 640): 38 token blocks = 5 groups; 64 samples halved to 16 slots (5 * 16 * 16 <= 6 * 256)
    p = ops.attn_plan(64, 1201, 16, (30, 40), stream_cus=256)
    assert (p.family, p.ww, p.groups, p.nbz, p.launches[0][1]) == (WIN, 40, 5, 16, (1280, 1, 1))
    p = ops.attn_plan(64, 1201, 16, (30, 40), backward=True, stream_cus=256)
    assert (p.family, p.groups, p.nbz, p.nbq) == (WIN, 5, 16, 16)
    assert [l[:2] for l in p.launches] == [("attn_stats_zero_kernel", (1, 1, 1)), ("attn_bwd_kv_win_kernel", (1280, 1, 1)),
                                          ("attn_bwd_q_win_kernel", (1280, 1, 1))]
    need = ops.attn_bwd_workspace(64, 1201, 16, (30, 40))
    assert need == 3187671040
    p = ops.attn_plan(64, 1201, 16, (30, 40), backward=True, ws=PTR, ws_bytes=need, stream_cus=256)
    assert p.family == WIN_DS and p.qs == 1280 and [l[0] for l in p.launches] == [
        "attn_stats_zero_kernel", "attn_win_stats_kernel", "attn_bwd_kvs_win_kernel", "attn_bwd_qs_win_kernel"]
    assert ops.attn_plan(64, 1201, 16, (30, 40), backward=True, ws=PTR, ws_bytes=need - 1, stream_cus=256).family == WIN
    assert ops.attn_plan(2, 321, 2, (16, 20), stream_cus=256).ww == 20
    assert ops.attn_plan(3, 324, 3, (17, 19), stream_cus=256).family == STREAM
    # more than 16 samples per slot: the kernel that owns the table gradient gets more slots.  B = 300, 2 groups x 2 heads
    # on 8 CUs: 300 halved to 10 slots (4 * 10 <= 48), 30 samples each; 19 slots hold 16
    p = ops.attn_plan(300, 321, 2, (16, 20), backward=True, stream_cus=8)
    assert (p.nbz, p.nbq) == (10, 19)
    assert ops.attn_plan(0, 197, 12, (14, 14), stream_cus=256).launches == []


def test_query_validates_like_the_call(ops):
    from mem_amd import _lib
    with pytest.raises(_lib.MemhipError, match="T must be window_h\\*window_w \\+ 1"):
        ops.attn_plan(4, 198, 12, (14, 14), stream_cus=256)
    with pytest.raises(_lib.MemhipError, match="attn_bwd: T must be"):
        ops.attn_plan(4, 198, 12, (14, 14), backward=True, stream_cus=256)
    with pytest.raises(_lib.MemhipError, match="head_dim must be 64"):
        ops.attn_plan(4, 197, 0, (14, 14), stream_cus=256)


# ---------------------------------------------------------------------------------------------------------------------------
# The cascade of commit 7f18427 (memhip_attn_fwd, memhip_attn_bwd_ws / _out_ws in attn.hip; attn16_fwd / attn16_bwd;
# launch_fwd / launch_bwd in attn_win.hip; attn_fwd_stream / attn_bwd_stream), transcribed statement by statement.  Returns
# (family, numbers, launches) or None where that code answered MEMHIP_EUNSUPPORTED.
def rel_len(Wh, Ww):
    off = (Wh - 1) * (2 * Ww - 1) + (Ww - 1)
    return (5 * off + 4 + 3) & ~3


W16, R16 = 14, 27
TABLEN16 = ((2 * ((W16 - 1) * R16 + (W16 - 1)) + 3) + ((W16 - 1) * R16 + 15) + 1 + 3) & ~3
IMG16, NB16 = 16 * W16 * 128, 16 * W16 // 32
LDS_FWD16 = (2 * TABLEN16 + 4) * 4 + 4 * IMG16 + NB16 * 4096
LDS_BWD16 = ((3 * TABLEN16 * 4 + 3 * 256 * 4 + 128 + 256 + 15) & ~15) + 4 * IMG16 + NB16 * 4096


def attn16_fits(T, Wh, Ww):
    return Wh == W16 and Ww == W16 and T == W16 * W16 + 1


def attn_win_fits(T, Wh, Ww):
    return T > 256 and Ww in (40, 20) and T == Wh * Ww + 1


def nwg16(B, H, cus):
    n = (cus if cus > 0 else 256) // H
    return 1 if n < 1 else min(n, B)


def pick_spb(B, H, cus):
    num_cu = cus if cus > 0 else 256
    for spb in range(1, 17):
        if ((B + spb - 1) // spb) * H <= num_cu:
            return spb
    return 16


def win_geo(WW):
    WS = (WW + 7) & ~7
    RPC = 128 // WS
    P = 2 * WW - 1
    return WS, RPC, P, ((RPC - 1) * P + WS + 8 + 3) & ~3


def parent_fwd(B, T, H, Wh, Ww, cus, o16, owin):
    if o16 and attn16_fits(T, Wh, Ww):
        nwg = nwg16(B, H, cus)
        return A16, dict(nwg=nwg), [("attn16_fwd_kernel", (nwg * H, 1, 1), 7 * 64 + 64, LDS_FWD16)]
    nkb = (T + 31) // 32
    TP = nkb * 32
    if nkb > 8:
        if owin and attn_win_fits(T, Wh, Ww):                                  # attn_fwd_win -> launch_fwd<WW>
            WS, RPC, P, CQ = win_geo(Ww)
            NB = (2 * Wh - 1) * P
            sm = (((NB + 3) & ~3) + CQ) * 4 + 4 * 128 * 128
            if sm <= KMAX:
                groups = (TP // 32 + 7) // 8
                nbz, per = B, groups * H
                while nbz > 1 and per * nbz > 6 * cus:
                    nbz = (nbz + 1) // 2
                grid = 8 * ((H * nbz + 7) // 8) * groups
                return WIN, dict(ww=Ww, groups=groups, nbz=nbz), [("attn_fwd_win_kernel", (grid, 1, 1), 512, sm)]
        CT = 128                                                               # attn_fwd_stream
        TPc = ((T + CT - 1) // CT) * CT
        sm = 4 * CT * 128 + (rel_len(Wh, Ww) + 2 * TPc) * 4 + 32
        if sm > KMAX:
            return None
        groups = (TP // 32 + 7) // 8
        return STREAM, dict(groups=groups), [("attn_fwd_stream_kernel", (groups, H, B), 512, sm)]
    spb = pick_spb(B, H, cus)
    sm = 4 * nkb * 32 * 128 + (rel_len(Wh, Ww) + 2 * nkb * 32) * 4 + 32
    if sm > KMAX:
        return None
    return SMALL, dict(n=nkb, spb=spb), [("attn_fwd_kernel", (((B + spb - 1) // spb) * H, 1, 1), 512, sm)]


def parent_bwd(B, T, H, Wh, Ww, cus, o16, owin, dtable, dv_bias, out, ws, ws_bytes):
    vbdt = dict(vb=int(dv_bias), dt=int(dtable))
    if o16 and not dv_bias and attn16_fits(T, Wh, Ww):
        nwg = nwg16(B, H, cus)
        return A16, dict(nwg=nwg, fd=int(out), **vbdt), [("attn16_bwd_kernel", (nwg * H, 1, 1), 7 * 64, LDS_BWD16)]
    L = []
    if out:                                                                    # memhip_attn_bwd with `out`: memhip_attn_delta first
        L.append(("attn_delta_kernel", ((B * T * H + 31) // 32, 1, 1), 256, 0))
    nkb = (T + 31) // 32
    TP = nkb * 32
    spb = pick_spb(B, H, cus)
    grid = ((B + spb - 1) // spb) * H
    glen = rel_len(Wh, Ww)
    if dtable:
        L.append(("attn_stats_zero_kernel", (1, 1, 1), 64, 0))
    if nkb > 8:
        if owin and attn_win_fits(T, Wh, Ww):                                  # attn_bwd_win -> launch_bwd<WW>
            WS, RPC, P, CQ = win_geo(Ww)
            NBP = ((2 * Wh - 1) * P + 3) & ~3
            groups = (TP // 32 + 7) // 8
            nbz, per = B, groups * H
            while nbz > 1 and per * nbz > 6 * cus:
                nbz = (nbz + 1) // 2
            nbq = nbz
            while (B + nbq - 1) // nbq > 16:
                nbq += 1
            QS = 128 * ((Wh + RPC - 1) // RPC)
            need = B * H * TP * QS * 2
            if owin == 1 and ws and ws_bytes >= need and (ws & 15) == 0:
                sm_kvs = (2 * (NBP + 2 * CQ) + 16 + 4 * 128 + 8 * 64) * 4 + 4 * 128 * 128
                sm_kvs0 = ((NBP + 2 * CQ) + 16 + 4 * 128 + 8 * 64) * 4 + 4 * 128 * 128
                sm_qs = 8 * 64 * 4 + 3 * 5 * 64 * 128
                if sm_kvs <= KMAX:
                    if dtable:
                        L.append(("attn_win_stats_kernel", (H * ((256 + H - 1) // H), 1, 1), 256, 0))
                    nb = nbq if dtable else nbz
                    L.append(("attn_bwd_kvs_win_kernel", (8 * ((H * nb + 7) // 8) * groups, 1, 1), 512, sm_kvs if dtable else sm_kvs0))
                    qgroups = (QS + 255) // 256
                    nbs = B
                    while nbs > 1 and qgroups * H * nbs > 6 * cus:
                        nbs = (nbs + 1) // 2
                    L.append(("attn_bwd_qs_win_kernel", (8 * ((H * nbs + 7) // 8) * qgroups, 1, 1), 512, sm_qs))
                    return WIN_DS, dict(ww=Ww, groups=groups, nbq=nb, nbs=nbs, qgroups=qgroups, qs=QS, **vbdt), L
            sm_kv = (NBP + CQ + 4 * 128 + 8 * 64) * 4 + 4 * 128 * 128
            sm_q = (2 * (NBP + CQ) + 8 * 64) * 4 + 4 * 128 * 128
            if not (sm_kv > KMAX or sm_q > KMAX):
                L.append(("attn_bwd_kv_win_kernel", (8 * ((H * nbz + 7) // 8) * groups, 1, 1), 512, sm_kv))
                L.append(("attn_bwd_q_win_kernel", (8 * ((H * nbq + 7) // 8) * groups, 1, 1), 512, sm_q))
                return WIN, dict(ww=Ww, groups=groups, nbz=nbz, nbq=nbq, **vbdt), L
        CTK, CTQ = 128, 64                                                     # attn_bwd_stream
        TPcK, TPcQ = ((T + CTK - 1) // CTK) * CTK, ((T + CTQ - 1) // CTQ) * CTQ
        sm_kv = 4 * CTK * 128 + (glen + 2 * TPcK + 4 * CTK + 64) * 4 + 32
        sm_q = 4 * CTQ * 128 + (2 * glen + 64 + 2 * TPcQ) * 4 + 32
        if sm_kv > KMAX or sm_q > KMAX:
            return None
        groups = (TP // 32 + 7) // 8
        L.append(("attn_bwd_kv_stream_kernel", (groups, H, B), 512, sm_kv))
        sspb = B * H * groups // 1024
        sspb = 1 if sspb < 1 else (16 if sspb > 16 else sspb)
        L.append(("attn_bwd_q_stream_kernel", (groups, H, (B + sspb - 1) // sspb), 512, sm_q))
        return STREAM, dict(groups=groups, stream_spb=sspb, **vbdt), L
    sm_kv = 4 * nkb * 32 * 128 + (glen + 6 * nkb * 32 + 64) * 4 + 32
    sm_q = 4 * nkb * 32 * 128 + (2 * glen + 64 + 2 * nkb * 32) * 4 + 32
    if sm_kv > KMAX or sm_q > KMAX:
        return None
    L += [("attn_bwd_kv_kernel", (grid, 1, 1), 512, sm_kv), ("attn_bwd_q_kernel", (grid, 1, 1), 512, sm_q)]
    return SMALL, dict(n=nkb, spb=spb, **vbdt), L


def parent_workspace(B, T, H, Wh, Ww):
    if not attn_win_fits(T, Wh, Ww):
        return 0
    WS, RPC, P, CQ = win_geo(Ww)
    return B * H * ((T + 31) // 32 * 32) * (128 * ((Wh + RPC - 1) // RPC)) * 2


def check_plan(ops, want, ctx, *a, **kw):
    from mem_amd import _lib
    if want is None:
        with pytest.raises(_lib.MemhipError, match="LDS"):
            ops.attn_plan(*a, **kw)
        return None
    p = ops.attn_plan(*a, **kw)
    family, numbers, launches = want
    assert p.family == family and p.launches == launches, (ctx, p.family, p.launches, want)
    for name, v in numbers.items():
        assert getattr(p, name) == v, (ctx, name, getattr(p, name), want)
    # never an empty grid, never more LDS than a workgroup can have
    for _, grid, block, lds in p.launches:
        assert min(grid) >= 1 and 64 <= block <= 512 and 0 <= lds <= KMAX, (ctx, p.launches)
    return p


def sweep(ops, options, cases, seed):
    """`cases` random calls per option setting, forward and backward each: the plan against the transcription.  Returns the
    families seen."""
    rng = np.random.default_rng(seed)
    seen = Counter()
    for o16, owin in OPTIONS:
        options(o16, owin)
        for _ in range(cases):
            B, H = int(rng.integers(1, 301)), int(rng.integers(1, 17))
            # every 4th window one the dedicated kernels take (14 x 14; 40 or 20 wide): a uniform draw hardly finds them
            pick = int(rng.integers(8))
            Wh, Ww = int(rng.integers(1, 41)), int(rng.integers(1, 41))
            if pick < 2:
                Wh, Ww = ((14, 14), (Wh, 40), (Wh, 20))[int(rng.integers(3))]
            elif pick == 2:   # beyond the issue's range, up to 400 rows: the windows at which the LDS sums stop fitting
                Wh, Ww = int(rng.integers(41, 401)), (40, 20, Ww)[int(rng.integers(3))]
            T = Wh * Ww + 1
            cus = CUS[int(rng.integers(6))]
            dtable, dv_bias, out = (bool(rng.integers(2)) for _ in range(3))
            need = parent_workspace(B, T, H, Wh, Ww)
            assert ops.attn_bwd_workspace(B, T, H, (Wh, Ww)) == need
            ws, ws_bytes = ((None, 0), (PTR, need), (PTR, need - 1), (PTR + 8, need), (PTR, need + 4096), (None, need))[int(rng.integers(6))]
            ctx = (o16, owin, B, H, Wh, Ww, cus, dtable, dv_bias, out, ws, ws_bytes)
            p = check_plan(ops, parent_fwd(B, T, H, Wh, Ww, cus, o16, owin), ctx, B, T, H, (Wh, Ww), stream_cus=cus)
            if p is not None:
                assert len(p.launches) == 1, ctx
            seen["fwd", p and p.family] += 1
            p = check_plan(ops, parent_bwd(B, T, H, Wh, Ww, cus, o16, owin, dtable, dv_bias, out, ws or 0, ws_bytes), ctx,
                           B, T, H, (Wh, Ww), backward=True, dtable=dtable, dv_bias=dv_bias, out=out, ws=ws, ws_bytes=ws_bytes,
                           stream_cus=cus)
            if p is not None:
                # the number of launches follows from the family and the flags
                aux = 0 if p.family == A16 else int(dtable) * (2 if p.family == WIN_DS else 1) + int(out)
                assert len(p.launches) == (1 if p.family == A16 else 2) + aux, ctx
            seen["bwd", p and p.family] += 1
    return seen


def test_plan_equals_the_parent_cascade(ops, options):
    """24 000 random calls (B 1..300, heads 1..16, windows 1..40 a side and an eighth of them up to 400 rows, CU counts {0, 8, 64, 248, 256, 304}, every flag, six
    workspace settings, options attn16 0 / 1 x attn_win 0 / 1 / 2), forward and backward: family, template choices,
    samples-per-workgroup numbers and the ordered launches equal what the cascade of 7f18427 did."""
    seen = sweep(ops, options, 4000, 20261018)
    # the sweep is not vacuous
    for key in [("fwd", f) for f in (A16, SMALL, WIN, STREAM)] + [("bwd", f) for f in (A16, SMALL, WIN, WIN_DS, STREAM)]:
        assert seen[key] >= 100, (key, seen)
    assert seen["fwd", WIN_DS] == 0 and seen["fwd", None] >= 100 and seen["bwd", None] >= 100
