"""What the I420 output costs a decoder, on one MI355X in one session.

    python tools/decodebench.py [--out DIR] [--splats 10000 50000] [--reps 5]
    python tools/decodebench.py --format 10:bt709:limited [--out DIR] [--splats 10000]
    python tools/decodebench.py --format 10:bt709:limited:422:planar 8:bt601:limited:420:semi ...

The workload is bench.py's ``video_decode`` (a GOP of 8 distinct 1920x1080
frame models, seed 4242) at 10k and again at 50k splats per frame.  Measured
(DESIGN.md §13d holds the figures):

1. ``render_frames_sum`` alone: the batched render as it was before the I420
   output existed, same build -- the baseline;
2. (1) + ``rgb_to_i420``: what ``decode_frames(output="i420")`` adds;
3. the conversion kernel alone, without and with a reference: its algorithmic
   bytes F*H*W*(12 + 1.5) (+1.5 with ref) over its time, as a share of 8 TB/s
   (the project's convention) and of the 6.29 TB/s float4-copy rate.  It
   rotates over three input batches (600 MB) so that the 256 MiB Infinity
   Cache cannot hold what it reads; in (2) the render has just written the
   images, and whatever the cache keeps of them there is the pipeline's own;
4. end to end, ``codec.decode_video`` of a 16-frame file to a .yuv on tmpfs
   against what a user did before: ``decode_frames`` -> ``.cpu()`` of the
   float images -> the same arithmetic in numpy on the host -> the file.

Every figure is the median of ``--reps`` windows between device events (4: a
host clock around work that ends in a synchronise), each window long enough
(--window seconds) to be past the clock's and the scheduler's grain, after a
warm-up of every shape; the variants of one comparison alternate window by
window, so drift in the shared host hits both.  Fails without a HIP device.

With ``--format DEPTH:MATRIX:RANGE`` the session measures that
pixel format (csrc/yuv_conv.hip's kernels with the format's table) against the legacy
8-bit one (the same kernels with the legacy constants) instead,
variant against variant in alternating windows: the output conversion alone
(without and with a reference) and behind ``render_frames_sum``, and the input
conversion per frame.  The yardstick is the legacy kernel's achieved bytes per
second in the same session, each kernel over its own algorithmic bytes per
pixel (12 + 1.5 samples' bytes, + 1.5 samples' with a reference).  With
``--format DEPTH:MATRIX:RANGE:CHROMA:LAYOUT`` (several may be
given) the kernels are the same source's instances of that layout and the yardstick is the
planar 4:2:0 instance of the same depth, matrix and range: 12 + 1.5 / 2 / 3 samples' bytes
per pixel at 4:2:0 / 4:2:2 / 4:4:4."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gsvc_amd import codec  # noqa: E402
from gsvc_amd import compress as C  # noqa: E402
from gsvc_amd.render import render_frames_sum  # noqa: E402
from gsvc_amd.video import YuvFormat, rgb_to_i420  # noqa: E402

H, W = 1080, 1920
PEAK_SPEC, PEAK_COPY = 8.0e12, 6.29e12


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
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        inner[name] = max(20, int(seconds * 1e6 / window_us(fn, 20)))
    got = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            got[name].append(window_us(fn, inner[name]))
    return {name: {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3),
                   "max_us": round(max(v), 3), "calls_per_window": inner[name]} for name, v in got.items()}


def gop_inputs(device, frames, splats):
    g = torch.Generator().manual_seed(4242)
    xyz = torch.atanh(2 * (torch.rand(frames * splats, 2, generator=g) - 0.5)).to(device)
    chol = torch.rand(frames * splats, 3, generator=g).to(device)
    feat = torch.rand(frames * splats, 3, generator=g).to(device)
    return xyz, chol, feat


def kernel_block(device, frames, splats, reps, seconds):
    xyz, chol, feat = gop_inputs(device, frames, splats)
    bound = torch.tensor([0.5, 0.0, 0.5], device=device)
    bg = torch.ones(3, device=device)
    sizes = [splats] * frames

    def render():
        return render_frames_sum(xyz, chol, feat, sizes, H, W, bg, cholesky_bound=bound)

    def render_i420():
        return rgb_to_i420(render())

    res = {"frames": frames, "splats": splats}
    res.update(compare({"render": render, "render_i420": render_i420}, reps, seconds))
    res["ratio"] = round(res["render_i420"]["median_us"] / res["render"]["median_us"], 4)

    # (3): three batches of images (the render's, shifted) and their own outputs
    base = render()
    batches = [base, (base * 0.5).contiguous(), (1.0 - base).contiguous()]
    refs = [rgb_to_i420(b.flip(0)) for b in batches]
    turn = [0]

    def convert():
        turn[0] = (turn[0] + 1) % 3
        return rgb_to_i420(batches[turn[0]])

    def convert_ref():
        turn[0] = (turn[0] + 1) % 3
        return rgb_to_i420(batches[turn[0]], refs[turn[0]])

    conv = compare({"convert": convert, "convert_ref": convert_ref}, reps, seconds)
    for name, per_pixel in (("convert", 13.5), ("convert_ref", 15.0)):
        nbytes = frames * H * W * per_pixel
        rate = nbytes / (conv[name]["median_us"] * 1e-6)
        conv[name].update(algorithmic_bytes=int(nbytes), tb_per_s=round(rate / 1e12, 3),
                          share_of_8tbs=round(rate / PEAK_SPEC, 3),
                          share_of_copy_rate=round(rate / PEAK_COPY, 3),
                          us_per_frame=round(conv[name]["median_us"] / frames, 3))
    res.update(conv)
    return res


def format_block(device, fmt, frames, splats, reps, seconds):
    """The kernels of ``fmt`` against their yardstick, in one session: the legacy
    8-bit kernels for a planar 4:2:0 format, the planar 4:2:0
    kernels of the same colour triple for any other chroma or layout (§13f)."""
    from gsvc_amd import _lib as L
    xyz, chol, feat = gop_inputs(device, frames, splats)
    bound = torch.tensor([0.5, 0.0, 0.5], device=device)
    bg = torch.ones(3, device=device)
    sizes = [splats] * frames
    yard = None if fmt.is_planar420 else YuvFormat(fmt.bit_depth, fmt.matrix, fmt.full_range)
    yname = "legacy" if fmt.is_planar420 else "planar420"

    def sample_bytes_per_pixel(f):
        return 1.5 if f is None else f.frame_bytes(H, W) / (H * W)

    def render():
        return render_frames_sum(xyz, chol, feat, sizes, H, W, bg, cholesky_bound=bound)

    res = {"format": str(fmt), "pix_fmt": fmt.pix_fmt, "yardstick": "legacy 8-bit I420" if yard is None else str(yard),
           "frames": frames, "splats": splats}
    behind = compare({"render_" + yname: lambda: rgb_to_i420(render(), fmt=yard),
                      "render_format": lambda: rgb_to_i420(render(), fmt=fmt)}, reps, seconds)
    behind["ratio"] = round(behind["render_format"]["median_us"] / behind["render_" + yname]["median_us"], 4)
    res["behind_render"] = behind

    # alone: three batches of images (600 MB: past the Infinity Cache) and their references
    base = render()
    batches = [base, (base * 0.5).contiguous(), (1.0 - base).contiguous()]
    refs = {yard: [rgb_to_i420(b.flip(0), fmt=yard) for b in batches],
            fmt: [rgb_to_i420(b.flip(0), fmt=fmt) for b in batches]}
    turn = [0]

    def convert(f, with_ref):
        def run():
            turn[0] = (turn[0] + 1) % 3
            return rgb_to_i420(batches[turn[0]], refs[f][turn[0]] if with_ref else None, fmt=f)
        return run

    def rates(got, pairs):
        for name, per_pixel, count in pairs:
            nbytes = count * H * W * per_pixel
            rate = nbytes / (got[name]["median_us"] * 1e-6)
            got[name].update(algorithmic_bytes=int(nbytes), tb_per_s=round(rate / 1e12, 3),
                             share_of_copy_rate=round(rate / PEAK_COPY, 3),
                             us_per_frame=round(got[name]["median_us"] / count, 3))

    by, bf = sample_bytes_per_pixel(yard), sample_bytes_per_pixel(fmt)
    out = compare({yname: convert(yard, False), "format": convert(fmt, False)}, reps, seconds)
    rates(out, ((yname, 12 + by, frames), ("format", 12 + bf, frames)))
    out["rate_ratio"] = round(out["format"]["tb_per_s"] / out[yname]["tb_per_s"], 4)
    res["output"] = out
    out = compare({yname: convert(yard, True), "format": convert(fmt, True)}, reps, seconds)
    rates(out, ((yname, 12 + 2 * by, frames), ("format", 12 + 2 * bf, frames)))
    out["rate_ratio"] = round(out["format"]["tb_per_s"] / out[yname]["tb_per_s"], 4)
    res["output_ref"] = out

    # input, one frame per call as load_yuv_frames does; 16 output slots (400 MB) in rotation
    slots = [torch.empty((1, 3, H, W), dtype=torch.float32, device=device) for _ in range(16)]
    stream = L.stream(device)

    def input_call(f):
        raw = refs[f][0]
        if f is None or f.is_legacy:
            def run():
                turn[0] = (turn[0] + 1) % 16
                L.call("gsvc_i420_to_rgb", L.ptr(raw[turn[0] % frames]), H, W, L.ptr(slots[turn[0]]), stream)
        elif f.is_planar420:
            c_fmt = f._c()

            def run():
                turn[0] = (turn[0] + 1) % 16
                L.call("gsvc_yuv420_to_rgb", 1, L.ptr(raw[turn[0] % frames]), H, W, c_fmt, L.ptr(slots[turn[0]]),
                       stream)
        else:
            c_fmt, chroma, semi = f._c(), int(f.chroma), int(f.layout == "semi")

            def run():
                turn[0] = (turn[0] + 1) % 16
                L.call("gsvc_yuv_to_rgb", 1, L.ptr(raw[turn[0] % frames]), H, W, c_fmt, chroma, semi,
                       L.ptr(slots[turn[0]]), stream)
        return run

    out = compare({yname: input_call(yard), "format": input_call(fmt)}, reps, seconds)
    rates(out, ((yname, 12 + by, 1), ("format", 12 + bf, 1)))
    out["rate_ratio"] = round(out["format"]["tb_per_s"] / out[yname]["tb_per_s"], 4)
    res["input"] = out
    return res


def _parse_format(text):
    parts = text.split(":")
    if len(parts) not in (3, 5) or parts[2] not in ("limited", "full"):
        raise SystemExit("--format is DEPTH:MATRIX:limited|full[:CHROMA:LAYOUT], e.g. 10:bt709:limited or "
                         "10:bt709:limited:422:planar")
    return YuvFormat(int(parts[0]), parts[1], parts[2] == "full", *parts[3:])


def _host_i420(rgb):
    """gsvc_rgb_to_i420's arithmetic (csrc/yuv_conv.hip) in numpy: what a user ran on the host."""
    f, _, h, w = rgb.shape
    c = np.fmin(np.fmax(rgb, np.float32(0)), np.float32(1))
    q = (c * np.float32(255) + np.float32(0.5)).astype(np.int32)
    y = (269484 * q[:, 0] + 528482 * q[:, 1] + 102760 * q[:, 2] + ((16 << 20) + (1 << 19))) >> 20
    s = q.reshape(f, 3, h // 2, 2, w // 2, 2).sum(axis=(3, 5), dtype=np.int32)
    u = (-155188 * s[:, 0] - 305135 * s[:, 1] + 460324 * s[:, 2] + ((128 << 22) + (1 << 21))) >> 22
    v = (460324 * s[:, 0] - 385875 * s[:, 1] - 74448 * s[:, 2] + ((128 << 22) + (1 << 21))) >> 22
    return np.concatenate([np.clip(p, 0, 255).astype(np.uint8).reshape(f, -1) for p in (y, u, v)], axis=1)


def video_streams(device, gops, frames, splats):
    """``gops`` GOPs of a key frame and frames - 1 deltas, untrained models."""
    torch.manual_seed(4242)
    kw = dict(H=H, W=W, BLOCK_H=16, BLOCK_W=16, device=device, lr=1e-3, quantize=True, opt_type="adan")
    streams = []
    for _ in range(gops):
        state = None
        for k in range(frames):
            if k == 0:
                m = C.GaussianVideoFrameQ(num_points=splats, **kw).to(device)
            else:
                m = C.GaussianVideoDelta(num_points=splats, **kw).to(device)
                with torch.no_grad():
                    m._xyz.copy_(0.02 * torch.randn(splats, 2))
                    m._cholesky.copy_(0.05 * torch.randn(splats, 3))
                    m._features_dc.copy_(0.05 * torch.randn(splats, 3))
                    m.p_xyz.copy_(state[0])
                    m.p_cholesky.copy_(state[1])
                    m.p_features_dc.copy_(state[2])
            m._init_data()
            m.eval()
            s = C.encode_frame(m, entropy=True)
            xq, _, cq, Lpre, _, _ = C.unpack_frames([s], device, prev=state)
            state = (xq, Lpre, cq)
            streams.append(s)
    return streams


def end_to_end(device, splats, reps, tmp):
    streams = video_streams(device, 2, 8, splats)
    path, out_new, out_old = (os.path.join(tmp, n) for n in ("v.gsvf", "new.yuv", "old.yuv"))
    codec.write_video(path, streams)
    vid = codec.read_video(path)

    def new():
        return codec.decode_video(path, out_new, device=device, batch=8)["seconds"]

    def old():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        state = None
        with open(out_old, "wb") as fh:
            for s in range(0, vid.num_frames, 8):
                imgs, state = C.decode_frames([vid.frame(i) for i in range(s, min(s + 8, vid.num_frames))],
                                              device, prev=state, return_state=True)
                fh.write(_host_i420(imgs.cpu().numpy()).tobytes())
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    new(), old()  # warm-up: every shape, the pinned buffers' first allocation, the page cache
    with open(out_new, "rb") as a, open(out_old, "rb") as b:
        same = a.read() == b.read()
    got = {"decode_video": [], "float_copy_and_numpy": []}
    for _ in range(reps):
        got["decode_video"].append(new())
        got["float_copy_and_numpy"].append(old())
    res = {"frames": vid.num_frames, "splats": splats, "file_bytes": vid.file_bytes,
           "outputs_equal": bool(same)}
    for name, v in got.items():
        res[name] = {"median_ms": round(1e3 * statistics.median(v), 3), "min_ms": round(1e3 * min(v), 3),
                     "max_ms": round(1e3 * max(v), 3),
                     "frames_per_s": round(vid.num_frames / statistics.median(v), 1)}
    res["speedup"] = round(res["float_copy_and_numpy"]["median_ms"] / res["decode_video"]["median_ms"], 2)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="directory for decodebench.json")
    ap.add_argument("--splats", type=int, nargs="+", default=[10000, 50000])
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds per timed window")
    ap.add_argument("--format", default=None, metavar="DEPTH:MATRIX:RANGE[:CHROMA:LAYOUT]", nargs="+",
                    help="measure these pixel formats' kernels against their yardstick instead, e.g. "
                         "10:bt709:limited (against the legacy kernels) or 10:bt709:limited:422:planar "
                         "(against planar 4:2:0 of the same depth)")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None,
                    help="where the end-to-end files go (tmpfs)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("decodebench: no HIP device (nothing is measured on the CPU)")
    device = torch.device("cuda:0")
    line = {"device": torch.cuda.get_device_name(0), "H": H, "W": W, "reps": args.reps,
            "window_s": args.window, "kernels": [], "end_to_end": []}
    if args.format:
        fmts = [_parse_format(text) for text in args.format]
        del line["kernels"], line["end_to_end"]
        line["formats"] = []
        with torch.no_grad():
            for fmt in fmts:
                for splats in args.splats:
                    line["formats"].append(format_block(device, fmt, args.frames, splats, args.reps, args.window))
                    print(json.dumps(line["formats"][-1]), flush=True)
        return _write(line, args.out)
    with torch.no_grad():
        for splats in args.splats:
            line["kernels"].append(kernel_block(device, args.frames, splats, args.reps, args.window))
            print(json.dumps(line["kernels"][-1]), flush=True)
        with tempfile.TemporaryDirectory(dir=args.tmp) as tmp:
            for splats in args.splats:
                line["end_to_end"].append(end_to_end(device, splats, args.reps, tmp))
                print(json.dumps(line["end_to_end"][-1]), flush=True)
    return _write(line, args.out)


def _write(line, out):
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "decodebench.json"), "w") as fh:
            json.dump(line, fh, indent=1)
            fh.write("\n")
    return line


if __name__ == "__main__":
    main()
