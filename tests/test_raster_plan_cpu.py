"""-m "not gpu": the dispatch of the event rasterizer (memhip_rasterize, one memhip_raster_args_t for every form), checked
through the plan query memhip_rasterize_plan.  The query takes the struct of the call (datasets.raster_args builds it), validates
and plans like the call itself and launches nothing."""
import ctypes as C
import itertools
from functools import lru_cache

import pytest

COUNT, FINALIZE, LDS_K, KEYS, ACCUM = "raster_count", "raster_finalize", "raster_lds_kernel", "raster_bin_keys", "raster_bin_accum"
KMAX = 160 * 1024      # LDS bytes a workgroup may use
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
AUTO, SINGLE, BINNED = 0, 1, 2

# the constants of csrc/raster.hip at commit 333d884
kThreads, kLdsThreads, kBandPixels, kMaxBands = 256, 1024, 14336, 6
kBinThreads, kBinEvPerThread, kBinMaxBands, kBinBandPixels, kAccThreads, kBinKeyGrid = 512, 8, 64, 40000, 1024, 4096
kBinChunk = kBinThreads * kBinEvPerThread
kBinSegs = 2 * kBinMaxBands
kBinHdr = kBinSegs + 1
kBinSlots = kBinChunk + 8 * kBinSegs
_BINNED_MAX_PIXELS = 64 * 40000                   # mem_amd/datasets.py


@pytest.fixture(scope="module")
def D():
    from mem_amd import datasets
    return datasets


@pytest.fixture
def options():
    """set(name, value); the defaults come back afterwards."""
    from mem_amd import _lib
    yield _lib.set_option
    _lib.set_option("raster_lds", 1)
    _lib.set_option("raster_bands", 0)


# ---------------------------------------------------------------------------------------------------------------------------
# The dispatch of commit 333d884, transcribed statement by statement: the rule of datasets.rasterize, the bodies of
# memhip_rasterize_aug_f64 / _var_f64 / _binned_f64 and of both workspace functions, bin_geometry and choose_bands (raster.hip).
# A launcher returns a return code (< 0) where that code answered with one, else a dict of what the plan holds.
def cdiv(a, b):
    return (a + b - 1) // b


def parent_rasterize_workspace(B, H, W):
    bins = B * 3 * H * W * 4
    bins = (bins + 15) & ~15
    return bins + B * 2 * 8


def parent_rasterize_binned_workspace(B, H, W, n_events):
    if B <= 0 or n_events < 0:
        return 0
    chunks = n_events // kBinChunk + B + 1
    keys = (chunks * kBinSlots * 2 + 15) & ~15
    hdr = chunks * kBinHdr * 4
    return keys + hdr + (kBinKeyGrid + B) * 4


def parent_bin_geometry(H, W, want_nb=0):
    HW = H * W
    n = (HW + kBinBandPixels - 1) // kBinBandPixels
    if want_nb > n and want_nb <= kBinMaxBands:
        n = want_nb
    if n > kBinMaxBands:
        return None
    px = (HW + n - 1) // n
    px = (px + 3) & ~3
    if px > kBinBandPixels:
        px = kBinBandPixels
        n = (HW + px - 1) // px
        if n > kBinMaxBands:
            return None
    return px, n


def parent_choose_bands(H, W, B, n_events, forced, max_cus):
    if forced > 0:
        return forced
    HW = H * W
    nmin = (HW + kBinBandPixels - 1) // kBinBandPixels
    cus = max_cus
    if cus <= 0:
        cus = 256
    if B * nmin <= cus:
        return nmin
    best, best_cost = nmin, 0.0
    nbv = nmin
    while nbv <= 2 * nmin + 4 and nbv <= kBinMaxBands:
        px = ((HW + nbv - 1) // nbv + 3) & ~3
        per_cu = 2 if px * 4 * 2 + 1024 <= 160 * 1024 else 1
        rounds = (B * nbv + cus * per_cu - 1) // (cus * per_cu)
        cost = float(rounds) * (0.22e-3 * float(px) + 220.0e-6 * (float(n_events) / B) / nbv) * (2.0 if per_cu == 2 else 1.0)
        if nbv == nmin or cost < best_cost * 0.9:
            best, best_cost = nbv, cost
        nbv += 1
    return best


def plan_dict(family, launches, ws, clears, rows_per_band=0, bands=0, band_px=0, nb=0, bx=0, offs=(0, 0, 0, 0, 0)):
    return dict(family=family, launches=launches, ws_bytes=ws, clears=clears, rows_per_band=rows_per_band, bands=bands,
                band_px=band_px, nb=nb, bx=bx, offs=offs)


EMPTY = plan_dict(None, [], 0, (0, 0, 0))


@lru_cache(maxsize=None)
def parent_aug_f64(B, H, W, time_surface, raster_lds, out_align):
    if not (B >= 0 and H > 0 and W > 0):
        return EINVAL
    if B == 0:
        return EMPTY
    need = parent_rasterize_workspace(B, H, W)
    bins_bytes = (B * 3 * H * W * 4 + 15) & ~15
    rpb = kBandPixels // W
    bands = cdiv(H, rpb) if rpb > 0 else kMaxBands + 1
    if raster_lds != 0 and not time_surface and bands <= kMaxBands and out_align % 4 == 0:
        rpb = cdiv(H, bands)
        return plan_dict("lds", [(LDS_K, bands, B, kLdsThreads, 2 * rpb * W * 4)], need, (0, B * 4, 0), rows_per_band=rpb,
                         bands=bands, offs=(0, bins_bytes, 0, 0, 0))
    bx = 8 if B >= 256 else (32 if B >= 32 else 256)
    fx = (H * W + kThreads - 1) // kThreads
    if fx > 64:
        fx = 64
    return plan_dict("global", [(COUNT, bx, B, kThreads, 0), (FINALIZE, fx, B, kThreads, 0)], need, (need, B * 4, 0),
                     offs=(0, bins_bytes, 0, 0, 0))


@lru_cache(maxsize=None)
def parent_var_f64(B, Hmax, Wmax, time_surface):
    if not (B >= 0 and Hmax > 0 and Wmax > 0):
        return EINVAL
    if B == 0:
        return EMPTY
    need = parent_rasterize_workspace(B, Hmax, Wmax)
    slot = Hmax * Wmax
    bins_bytes = (B * 3 * slot * 4 + 15) & ~15
    bx = 8 if B >= 256 else (32 if B >= 32 else 256)
    fx = (slot + kThreads - 1) // kThreads
    if fx > 64:
        fx = 64
    return plan_dict("global_var", [(COUNT, bx, B, kThreads, 0), (FINALIZE, fx, B, kThreads, 0)], need, (need, B * 4, B * 3 * slot),
                     offs=(0, bins_bytes, 0, 0, 0))


@lru_cache(maxsize=None)
def parent_binned_f64(B, H, W, n_events, raster_bands, max_cus, out_align):
    if not (B >= 0 and H > 0 and W > 0 and n_events >= 0):
        return EINVAL
    if B == 0:
        return EMPTY
    if out_align % 4:
        return EINVAL
    g = parent_bin_geometry(H, W, parent_choose_bands(H, W, B, n_events, raster_bands, max_cus))
    if g is None:
        return EUNSUPPORTED
    band_px, nb = g
    need = parent_rasterize_binned_workspace(B, H, W, n_events)
    keys_bytes = ((n_events // kBinChunk + B + 1) * kBinSlots * 2 + 15) & ~15
    chunk_slots = n_events // kBinChunk + B + 1
    bad_slots = keys_bytes + chunk_slots * kBinHdr * 4
    avg_chunks = n_events // (B * kBinChunk) + 1
    bx = (kBinKeyGrid + B - 1) // B
    if bx > 4 * avg_chunks:
        bx = 4 * avg_chunks
    if bx < 1:
        bx = 1
    return plan_dict("binned", [(KEYS, bx, B, kBinThreads, 0), (ACCUM, nb, B, kAccThreads, band_px * 4)], need, (0, 0, 0),
                     band_px=band_px, nb=nb, bx=bx, offs=(0, 0, 0, keys_bytes, bad_slots))


def parent(B, H, W, time_surface, dims, form, raster_lds, raster_bands, n_events, cus, out_align):
    """What the parent's Python did with these arguments.  mem_amd/augment.py called memhip_rasterize_var_f64 for per-sample
    canvases; datasets.rasterize(binned=None / False / True) is AUTO / SINGLE / BINNED.  BINNED with a time surface or dims is
    MEMHIP_EINVAL now (the parent dropped the time surface silently and had no such call for dims)."""
    if form == BINNED and (time_surface or dims):
        return EINVAL
    if dims:
        return parent_var_f64(B, H, W, time_surface)
    binned = {AUTO: None, SINGLE: False, BINNED: True}[form]
    if binned is None:
        binned = not time_surface and B > 0 and H * W <= _BINNED_MAX_PIXELS
    if binned:
        return parent_binned_f64(B, H, W, n_events, raster_bands, cus, out_align)
    return parent_aug_f64(B, H, W, time_surface, raster_lds, out_align)


def got_dict(p):
    return dict(family=p.family_name, launches=p.launches, ws_bytes=p.ws_bytes,
                clears=(p.clear_ws_bytes, p.clear_status_bytes, p.clear_out_bytes), rows_per_band=p.rows_per_band, bands=p.bands,
                band_px=p.band_px, nb=p.nb, bx=p.bx, offs=(p.off_bins, p.off_tstat, p.off_keys, p.off_hdr, p.off_bad_slots))


def check_invariants(got, B, H, W, n_events, ctx):
    """What the launcher and the kernels rely on."""
    HW = H * W
    if got["family"] == "binned":
        px, nb = got["band_px"], got["nb"]
        assert px % 4 == 0 and 0 < px <= kBinBandPixels and 1 <= nb <= kBinMaxBands, ctx
        assert (nb - 1) * px < HW <= nb * px, ctx                      # every band non-empty, the bands tile [0, H*W)
        assert got["bx"] >= 1 and got["bx"] * B <= kBinKeyGrid + B, ctx
        _, _, keys, hdr, bad = got["offs"]
        chunks = n_events // kBinChunk + B + 1                        # every sample starts a chunk of its own
        # keys are read 16 bytes per lane and the headers follow them at a 16-byte boundary; a chunk's header is 129 words, so
        # the per-workgroup slots behind the headers (int32, one plain store / load each) start at a 4-byte boundary
        assert keys == 0 and hdr % 16 == 0 and bad % 4 == 0, ctx
        assert hdr - keys >= chunks * kBinSlots * 2 and bad - hdr >= chunks * kBinHdr * 4, ctx
        assert got["ws_bytes"] >= bad + got["bx"] * B * 4, ctx
    elif got["family"] is not None:
        bins, tstat = got["offs"][:2]
        assert bins == 0 and tstat % 16 == 0 and tstat >= B * 3 * HW * 4 and got["ws_bytes"] >= tstat + B * 2 * 8, ctx
        if got["family"] == "lds":
            rpb, bands = got["rows_per_band"], got["bands"]
            assert 1 <= bands <= kMaxBands and (bands - 1) * rpb < H <= bands * rpb and rpb * W <= kBandPixels, ctx
    assert (got["family"] is None) == (B == 0) == (not got["launches"]), ctx
    for _, gx, gy, block, lds in got["launches"]:
        assert gx * gy >= 1 and gy == B and block in (256, 512, 1024) and 0 <= lds <= KMAX, ctx


GRID = dict(
    B=(0, 1, 2, 31, 32, 33, 64, 255, 256, 300),
    canvas=((1, 1), (2, 3), (5, 7), (37, 1000), (180, 240), (224, 224), (480, 640), (1600, 1600), (1601, 1600)),
    time_surface=(0, 1), dims=(False, True), form=(AUTO, SINGLE, BINNED), raster_lds=(0, 1),
    raster_bands=(0, 1, 2, 10, 13, 16, 40, 64, 65), n_events=(0, 1, 4095, 4096, "30000B", "1000000B"), cus=(8, 64, 256, 304),
    out_align=(1, 4))


def test_plan_equals_the_parent_dispatch(D, options):
    """The whole grid GRID (933 120 structs): family, geometry, every launch's grid / block / LDS, clears, workspace
    bytes and layout and bx equal the transcription, return codes included.  The one exception is the corrected band count:
    where the parent's trailing bands were empty ((nb - 1) * band_px >= H * W) the plan keeps band_px and has
    nb = ceil(H * W / band_px); that set is not empty, and confined to canvases below 4 * 64 pixels or forced band counts."""
    from mem_amd import _lib
    lib = _lib.lib
    plan = D.RasterPlan()
    pplan = C.byref(plan)
    seen, corrected, total = {}, set(), 0
    for raster_lds, raster_bands in itertools.product(GRID["raster_lds"], GRID["raster_bands"]):
        options("raster_lds", raster_lds)
        options("raster_bands", raster_bands)
        for B, (H, W), ts, dims, form, n_ev, cus, align in itertools.product(
                GRID["B"], GRID["canvas"], GRID["time_surface"], GRID["dims"], GRID["form"], GRID["n_events"], GRID["cus"],
                GRID["out_align"]):
            n_events = int(n_ev[:-1]) * B if isinstance(n_ev, str) else n_ev
            ctx = (B, H, W, ts, dims, form, raster_lds, raster_bands, n_events, cus, align)
            want = parent(*ctx)
            a = D.raster_args(B, H, W, ts, form, n_events, dims=16 if dims else None, out=0x1000 + align % 4)
            rc = lib.memhip_rasterize_plan(C.byref(a), cus, pplan)
            total += 1
            if isinstance(want, int):
                assert rc == want, (ctx, rc, lib.memhip_last_error())
                seen[want] = seen.get(want, 0) + 1
                continue
            assert rc == 0, (ctx, rc, lib.memhip_last_error())
            got = got_dict(plan)
            seen[got["family"]] = seen.get(got["family"], 0) + 1
            check_invariants(got, B, H, W, n_events, ctx)
            if want["family"] == "binned" and (want["nb"] - 1) * want["band_px"] >= H * W:
                corrected.add(ctx)
                assert H * W < 4 * 64 or raster_bands > 0, ctx
                nb = cdiv(H * W, want["band_px"])
                assert nb < want["nb"]
                want = dict(want, nb=nb, launches=[want["launches"][0], (ACCUM, nb, B, kAccThreads, want["band_px"] * 4)])
            assert got == want, (ctx, got, want)
    assert total == 933120
    assert corrected and {c[1:3] for c in corrected} >= {(2, 3), (5, 7)}
    # not vacuous: every family, the empty batch and the three return codes
    for k in ("binned", "lds", "global", "global_var", None, EINVAL, EUNSUPPORTED):
        assert seen.get(k, 0) >= 1000, (k, seen)


def test_worked_numbers(D, options):
    """256 CUs, default options."""
    def plan(B, H, W, n, ts=False, form=AUTO, dims=None):
        return D.raster_plan(D.raster_args(B, H, W, ts, form, n, dims=dims), 256)
    # BASELINE configs[3]: 32 x 1 M events on 480 x 640: eight bands of 38 400 pixels, 256 pass-2 workgroups = one round
    p = plan(32, 480, 640, 32_000_000)
    assert (p.family_name, p.band_px, p.nb, p.bx) == ("binned", 38400, 8, 128)
    assert p.launches == [(KEYS, 128, 32, 512, 0), (ACCUM, 8, 32, 1024, 153600)]
    assert (p.clear_ws_bytes, p.clear_status_bytes, p.clear_out_bytes) == (0, 0, 0)
    chunks = 32_000_000 // 4096 + 33
    assert (p.off_hdr, p.off_bad_slots, p.ws_bytes) == (chunks * 5120 * 2, chunks * (5120 * 2 + 129 * 4), chunks * 10756 + 4128 * 4)
    # 64 samples: two rounds either way, the model keeps the eight bands
    assert plan(64, 480, 640, 64_000_000).nb == 8
    # the pretraining batch: 256 x 30 000 events on 224 x 224
    p = plan(256, 224, 224, 256 * 30000)
    assert (p.family_name, p.nb, p.bx) == ("binned", 2, 16) and p.band_px == 224 * 112
    # the single-pass forms of the same batch: four bands of 56 rows in LDS; the time surface takes the global atomics
    p = plan(256, 224, 224, 256 * 30000, form=SINGLE)
    assert (p.family_name, p.rows_per_band, p.bands) == ("lds", 56, 4) and p.launches == [(LDS_K, 4, 256, 1024, 2 * 56 * 224 * 4)]
    assert (p.clear_ws_bytes, p.clear_status_bytes) == (0, 1024)
    p = plan(256, 224, 224, 256 * 30000, ts=True)
    assert p.family_name == "global" and p.launches == [(COUNT, 8, 256, 256, 0), (FINALIZE, 64, 256, 256, 0)]
    assert p.clear_ws_bytes == p.ws_bytes == 256 * 3 * 224 * 224 * 4 + 256 * 16 and p.off_tstat == 256 * 3 * 224 * 224 * 4
    options("raster_lds", 0)
    assert plan(256, 224, 224, 0, form=SINGLE).family_name == "global"
    options("raster_lds", 1)
    # per-sample canvases: the global form, and the slots are cleared
    p = plan(4, 260, 346, 1000, dims=16)
    assert p.family_name == "global_var" and p.clear_out_bytes == 4 * 3 * 260 * 346 and p.launches[0] == (COUNT, 256, 4, 256, 0)
    # the corrected geometry: 35 pixels in 64 forced bands are 9 bands of 4 pixels, not 64 of which 55 start behind the canvas
    options("raster_bands", 64)
    p = plan(3, 5, 7, 100)
    assert (p.band_px, p.nb) == (4, 9) and p.launches[1] == (ACCUM, 9, 3, 1024, 16)
    options("raster_bands", 0)
    assert plan(0, 5, 7, 0).launches == [] and plan(0, 5, 7, 0).family == 0


def test_device_cus_default_is_256(D):
    """A device that reports no CU count plans like one of 256 (choose_bands always assumed so)."""
    a = D.raster_args(300, 480, 640, False, BINNED, 300 * 10 ** 6)
    assert got_dict(D.raster_plan(a, 0)) == got_dict(D.raster_plan(a, 256))
