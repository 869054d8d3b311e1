"""Which kernels does the rasterizer launch for a batch?  Prints what datasets.raster_plan names for a shape: the kernel family,
its bands, the workspace bytes with the offsets of its parts, what is cleared in front of the launches, and per launch the
kernel, grid in workgroups, workgroup size and LDS bytes.  Nothing is launched; with --cus no device is needed.

    python tools/raster_launch_list.py --batch 32 --canvas 480 640 --events 1000000 --cus 256          # BASELINE configs[3]
    python tools/raster_launch_list.py --batch 256 --canvas 224 224 --events 30000 --form single      # the LDS family
    python tools/raster_launch_list.py --batch 4 --canvas 260 346 --events 50000 --dims --time-surface
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mem_amd import _lib, datasets as D                                   # noqa: E402

FORMS = {"auto": D.RASTER_AUTO, "single": D.RASTER_SINGLE, "binned": D.RASTER_BINNED}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--canvas", type=int, nargs=2, default=(480, 640), metavar=("H", "W"))
    ap.add_argument("--events", type=int, default=1_000_000, help="events per sample (n_events = batch x this)")
    ap.add_argument("--form", choices=sorted(FORMS), default="auto")
    ap.add_argument("--time-surface", action="store_true")
    ap.add_argument("--dims", action="store_true", help="per-sample canvases (--canvas is then the largest)")
    ap.add_argument("--cus", type=int, default=None, help="CUs of the device (default: ask the current one)")
    ap.add_argument("--raster-lds", type=int, default=None, help="the raster_lds option (default: the library's)")
    ap.add_argument("--raster-bands", type=int, default=None, help="the raster_bands option (default: the library's)")
    a = ap.parse_args()
    for name, v in (("raster_lds", a.raster_lds), ("raster_bands", a.raster_bands)):
        if v is not None:
            _lib.set_option(name, v)
    H, W = a.canvas
    p = D.raster_plan(D.raster_args(a.batch, H, W, a.time_surface, FORMS[a.form], a.batch * a.events, dims=16 if a.dims else None),
                      a.cus)
    print(f"batch {a.batch}, canvas {H}x{W}{' (per-sample)' if a.dims else ''}, {a.events} events per sample, form {a.form}"
          f"{', time surface' if a.time_surface else ''}, raster_lds {_lib.get_option('raster_lds')}, raster_bands "
          f"{_lib.get_option('raster_bands')}, {'device' if a.cus is None else a.cus} CUs")
    geometry = {"lds": f"{p.bands} bands of {p.rows_per_band} rows", "binned": f"{p.nb} bands of {p.band_px} pixels, bx {p.bx}"}
    print(f"family {p.family_name}  {geometry.get(p.family_name, '')}")
    parts = {"binned": (("keys", p.off_keys), ("hdr", p.off_hdr), ("bad_slots", p.off_bad_slots))}.get(
        p.family_name, (("bins", p.off_bins), ("tstat", p.off_tstat)))
    print(f"workspace {p.ws_bytes} bytes  " + "  ".join(f"{n} @ {o}" for n, o in parts))
    print(f"cleared: workspace {p.clear_ws_bytes}  status {p.clear_status_bytes}  out {p.clear_out_bytes}")
    for kernel, gx, gy, block, lds in p.launches:
        print(f"{kernel:18s} grid {gx:5d} x {gy:<5d} x {block}  lds {lds}")


if __name__ == "__main__":
    main()
