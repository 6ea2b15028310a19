"""What a view costs the batched render, on one MI355X in one session.

    python tools/resamplebench.py [--out DIR] [--splats 50000] [--reps 5]
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/resamplebench.py --trace
    python tools/resamplebench.py --summarize DIR

The workload is a GOP of 8 distinct 1920x1080 frame models (seed 4242) of
``--splats`` splats each, their Cholesky factors scaled (``--chol-scale``) to a
trained frame's density (about 97 entries per tile at 50k, README; the session
prints the density it got from the render's own M).  Measured, variant against
variant in alternating windows (DESIGN.md §13g holds the figures):

    native     ``render_frames_sum`` as it is without a view
    identity   the same through an identity ``View`` (the resampled composite
               at the native samples: what the generic kernel costs)
    up2        3840x2160
    half       960x540
    crop       the centre quarter of the frame (960x540 source pixels) at
               1920x1080
    quarter    480x270, point-sampled
    half_aa2   960x540 with ``aa=2``: the filtered composite
    quarter_aa4  480x270 with ``aa=4``
    half_2pass, quarter_2pass
               the two-pass baseline of each ``aa`` variant, what there was
               before the filtered composite: the fine point-sampled view into
               a temporary, then ``torch.nn.functional.avg_pool2d``

Every figure is the median of ``--reps`` (at least 5) windows between device
events, each ``--window`` seconds long, after a warm-up of every shape.  A row
also gives the composite's lane use from the view's tables -- samples over 64 x
the 64-sample chunks the tiles walk -- and the share of source tiles that own
no sample; for an ``aa`` view the lane use of the filtered composite's trips
and its seam pixels (the output pixels that straddle a tile edge).  ``--trace`` runs ``--trace-calls`` calls of each variant and
nothing else: the run to put under ``rocprofv3 --kernel-trace``, whose kernel
table splits a call into projection and composite (``--summarize DIR`` reads
it back per variant).  Fails without a HIP device."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gsvc_amd.render import View, render_frames_sum  # noqa: E402

H, W = 1080, 1920


def window_us(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / inner


def compare(variants, reps, seconds):
    """{name: fn} -> {name: median / min / max microseconds per call}; windows alternate."""
    inner = {}
    for name, fn in variants.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        inner[name] = max(5, int(seconds * 1e6 / window_us(fn, 5)))
    got = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            got[name].append(window_us(fn, inner[name]))
    return {name: {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3),
                   "max_us": round(max(v), 3), "calls_per_window": inner[name]} for name, v in got.items()}


def lane_use(view):
    """(busy lanes / lanes issued, share of tiles without a sample) of the
    composite's flat 64-sample chunks, from the view's tables."""
    rows = np.diff(view.row_start).astype(np.int64)[:, None]
    cols = np.diff(view.col_start).astype(np.int64)[None, :]
    samples = rows * cols
    chunks = (samples + 63) // 64
    return float(samples.sum()) / float(64 * chunks.sum()), float((samples == 0).mean())


def lane_use_aa(view):
    """(busy lanes / lanes issued, seam pixels, output pixels) of the filtered
    composite, from the fine view's tables: a tile touches the output pixels
    that hold one of its sub-samples and walks them floor(64 / (ky kx)) a trip."""
    ky, kx = view.aa
    per_trip = 64 // (ky * kx)
    rs, cs = view.fine.row_start.astype(np.int64), view.fine.col_start.astype(np.int64)
    own_r, own_c = (rs[1:] > rs[:-1]), (cs[1:] > cs[:-1])
    pr = np.where(own_r, (rs[1:] - 1) // ky + 1 - rs[:-1] // ky, 0)[:, None]
    pc = np.where(own_c, (cs[1:] - 1) // kx + 1 - cs[:-1] // kx, 0)[None, :]
    trips = (pr * pc + per_trip - 1) // per_trip
    seam_r = int(((rs[1:-1] % ky) != 0).sum())  # a tile range that starts inside a pixel
    seam_c = int(((cs[1:-1] % kx) != 0).sum())
    seam = seam_r * view.out_w + seam_c * view.out_h - seam_r * seam_c
    samples = float(view.fine.out_h) * float(view.fine.out_w)
    return samples / float(64 * trips.sum()), seam, view.out_h * view.out_w


VARIANTS = ["native", "identity", "up2", "half", "crop", "quarter", "half_aa2", "half_2pass", "quarter_aa4",
            "quarter_2pass"]
_CLASSES = (("projection_us", ("frame_project_kernel",)),
            ("composite_us", ("raster_resampled_kernel", "raster_sum_fwd_kernel", "raster_filtered_kernel")),
            ("seams_us", ("filter_seams_kernel",)), ("pool_us", ("avg_pool", "AvgPool")))


def summarize(trace_dir, calls):
    """The kernel table of a ``--trace`` run under rocprofv3 (csv): per variant,
    in the order it ran, the median microseconds per call of the projection,
    the composite, the filtered composite's seam kernel and the two-pass
    baseline's pooling kernel over its last ``calls`` calls.  A call begins at
    its projection kernel."""
    import csv
    import glob
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as fh:
            rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"])
                     for r in csv.DictReader(fh)]
    rows.sort()
    per_call = []
    for s, e, k in rows:
        if "frame_project_kernel" in k:
            per_call.append({})
        if not per_call:
            continue
        for key, words in _CLASSES:
            if any(w in k for w in words):
                per_call[-1][key] = per_call[-1].get(key, 0.0) + (e - s) / 1e3
    per = len(per_call) // len(VARIANTS)
    out = {}
    for i, name in enumerate(VARIANTS):
        mine = per_call[i * per:(i + 1) * per][-calls:]
        out[name] = {key: round(statistics.median(c.get(key, 0.0) for c in mine), 2) for key, _ in _CLASSES
                     if any(key in c for c in mine)}
        out[name]["calls"] = len(mine)
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--summarize", default=None, metavar="DIR",
                    help="read the kernel trace rocprofv3 left in DIR for a --trace run and print the "
                         "composite's and the projection's time per variant (no device needed)")
    ap.add_argument("--out", default=None, help="directory for resamplebench.json")
    ap.add_argument("--splats", type=int, default=50000)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--chol-scale", type=float, default=8.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds per timed window")
    ap.add_argument("--trace", action="store_true", help="a few calls per variant, no timing")
    ap.add_argument("--trace-calls", type=int, default=5)
    args = ap.parse_args(argv)
    if args.summarize:
        return summarize(args.summarize, args.trace_calls)
    if not torch.cuda.is_available():
        raise SystemExit("resamplebench: no HIP device (nothing is measured on the CPU)")
    if args.reps < 5:
        raise SystemExit("resamplebench: at least 5 windows")
    device = torch.device("cuda:0")
    F, n = args.frames, args.splats
    g = torch.Generator().manual_seed(4242)
    xyz = torch.atanh(2 * (torch.rand(F * n, 2, generator=g) - 0.5)).to(device)
    chol = (torch.rand(F * n, 3, generator=g) * args.chol_scale).to(device)
    feat = (torch.rand(F * n, 3, generator=g) * 0.05).to(device)
    bound = torch.tensor([0.5, 0.0, 0.5], device=device)
    bg = torch.ones(3, device=device)
    sizes = [n] * F
    views = {"native": None, "identity": View(H, W), "up2": View(H, W, size=(2 * H, 2 * W)),
             "half": View(H, W, size=(H // 2, W // 2)),
             "crop": View(H, W, size=(H, W), crop=(W // 4, H // 4, W // 2, H // 2)),
             "quarter": View(H, W, size=(H // 4, W // 4)),
             "half_aa2": View(H, W, size=(H // 2, W // 2), aa=2),
             "half_2pass": View(H, W, size=(H // 2, W // 2), aa=2),
             "quarter_aa4": View(H, W, size=(H // 4, W // 4), aa=4),
             "quarter_2pass": View(H, W, size=(H // 4, W // 4), aa=4)}
    assert list(views) == VARIANTS

    def render(view):
        return render_frames_sum(xyz, chol, feat, sizes, H, W, bg, cholesky_bound=bound, view=view)

    def call(view, two_pass=False):
        if two_pass:  # the fine view into a temporary, then the box mean by torch
            return lambda: torch.nn.functional.avg_pool2d(render(view.fine), view.aa)
        return lambda: render(view)

    calls = {name: call(view, name.endswith("_2pass")) for name, view in views.items()}

    with torch.no_grad():
        if args.trace:
            for name in views:
                for _ in range(args.trace_calls):
                    calls[name]()
                torch.cuda.synchronize()
            print(json.dumps({"trace_calls": args.trace_calls, "order": list(views)}), flush=True)
            return None
        same = bool(torch.equal(call(None)(), call(views["identity"])()))
        # float32 pooling sums in another order than the rule: close, not equal
        aa_err = {name: float((calls[name]() - calls[name.replace("_aa2", "_2pass").replace("_aa4", "_2pass")]())
                              .abs().max()) for name in ("half_aa2", "quarter_aa4")}
        from gsvc_amd import render as R
        bw = next(iter(R._batch_workspaces.values()))
        m = int(bw.meta[:, 0].sum())
        line = {"device": torch.cuda.get_device_name(0), "H": H, "W": W, "frames": F, "splats": n,
                "chol_scale": args.chol_scale, "entries_per_tile": round(m / (F * 68 * 120), 2),
                "identity_equals_native": same, "max_abs_fused_minus_two_pass": aa_err, "reps": args.reps,
                "window_s": args.window}
        res = compare(calls, args.reps, args.window)
        for name, view in views.items():
            if name.endswith("_2pass"):  # the composite of the fine view, point-sampled
                use, empty = lane_use(view.fine)
                res[name].update(out=[view.out_h, view.out_w], aa=list(view.aa), lane_use=round(use, 4),
                                 temporary_bytes=4 * F * 3 * view.fine.out_h * view.fine.out_w)
                fused = res[name.replace("half_2pass", "half_aa2").replace("quarter_2pass", "quarter_aa4")]
                fused["vs_two_pass"] = round(fused["median_us"] / res[name]["median_us"], 3)
                fused["inside_two_pass_range"] = bool(fused["median_us"] <= res[name]["max_us"])
            elif view is not None and view.aa != (1, 1):
                use, seam, pixels = lane_use_aa(view)
                res[name].update(out=[view.out_h, view.out_w], aa=list(view.aa), lane_use=round(use, 4),
                                 seam_pixels=seam, seam_share=round(seam / pixels, 4))
            elif view is not None:
                use, empty = lane_use(view)
                res[name].update(out=[view.out_h, view.out_w], lane_use=round(use, 4),
                                 tiles_without_samples=round(empty, 4))
            res[name]["us_per_frame"] = round(res[name]["median_us"] / F, 3)
            res[name]["vs_native"] = round(res[name]["median_us"] / res["native"]["median_us"], 3)
        line["variants"] = res
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "resamplebench.json"), "w") as fh:
            json.dump(line, fh, indent=1)
            fh.write("\n")
    return line


if __name__ == "__main__":
    main()
