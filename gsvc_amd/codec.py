"""The codec's file and its decoder: ``.yuv -> models -> one file -> .yuv``.

``compress.encode_frame`` gives one byte string per frame; this module puts a
video's frame streams into ONE file with an index (``write_video`` /
``read_video``), decodes such a file -- or a list of streams -- to raw YUV
(8-bit I420 by default; 8 to 16 bits, BT.601 or BT.709, limited or full range,
4:2:0 / 4:2:2 / 4:4:4, planar or semi-planar as NV12 / P010:
``video.YuvFormat``) in batches on the GPU (``decode_video``:
``decode_frames(output="i420")``, csrc/yuv_conv.hip), and is the command line of the three steps:

    python -m gsvc_amd.codec encode MODELS.pth SRC.yuv OUT.gsvf --width W --height H
    python -m gsvc_amd.codec info OUT.gsvf
    python -m gsvc_amd.codec decode OUT.gsvf OUT.yuv [--reference SRC.yuv]
                                    [--size WxH] [--crop X,Y,W,H] [--aa auto|K|KYxKX]

Not part of the reference, which writes PNG images and an MP4 through OpenCV
(train_video_Compress.py) and has no bitstream file.

The container, little-endian:

    bytes 0-63      "GSVF", u32 version 1, u32 H, u32 W, u32 num_frames,
                    u32 fps_num, u32 fps_den, u32 flags, u64 index_offset,
                    u64 file_bytes, u32 layout, zero to 64; flags: the
                    source's pixel format (video.YuvFormat): bits 0-1 depth (0: 8, 1: 10,
                    2: 12, 3: 16 bits), bit 4 matrix (0 bt601, 1 bt709),
                    bit 6 full range, every other bit 0 (files written
                    before the format existed have flags 0: 8-bit BT.601
                    limited range); layout (byte 48, the first byte that
                    was reserved): bits 0-1 chroma (0: 4:2:0, 1: 4:2:2,
                    2: 4:4:4), bit 4 semi-planar (interleaved U, V), every
                    other bit 0 (files written before read as planar 4:2:0)
    64 ...          the frame streams of encode_frame (version 1 or 2, any
                    mix), back to back
    index_offset... per frame: u64 offset, u32 length, u32 flags (bit 0: delta,
                    copied from the frame header)

Frame indices of this module (``frame(i)``, ``span(i)``, ``key_frames``,
``frames=range(a, b)``) count from 0; ``compress_video``'s ``K_frames`` and the
``--k_frames`` option count from 1, as the reference's K_frames.txt.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import struct
import time
from typing import List, Optional, Sequence

import numpy as np
import torch

from .compress import FLAG_DELTA, HEADER_BYTES, decode_frames, parse_header
from .video import YuvFormat, add_format_arguments, format_of_arguments

FILE_MAGIC = b"GSVF"
FILE_VERSION = 1
FILE_HEADER_BYTES = 64
INDEX_ENTRY_BYTES = 16
_FILE_HEADER = struct.Struct("<4sIIIIIIIQQ")  # magic .. file_bytes: 48 bytes, zero to 64
_LAYOUT_WORD = struct.Struct("<I")  # at byte 48: YuvFormat.layout_code
_INDEX_ENTRY = struct.Struct("<QII")


def _check_sequence(heads: Sequence[dict], H: Optional[int] = None, W: Optional[int] = None) -> None:
    """What spans frames: one size, frame 0 a key frame, a delta no larger
    than the frame before it.  ValueError."""
    if not heads:
        raise ValueError("a video has at least one frame")
    if H is None:
        H, W = heads[0]["H"], heads[0]["W"]
    for i, h in enumerate(heads):
        if (h["H"], h["W"]) != (H, W):
            raise ValueError(f"frame {i} is {h['H']}x{h['W']}, the video {H}x{W}")
        if h["delta"] and i == 0:
            raise ValueError("frame 0 is a delta frame: nothing to add it to")
        if h["delta"] and h["N"] > heads[i - 1]["N"]:
            raise ValueError(f"delta frame {i} has {h['N']} splats, its predecessor {heads[i - 1]['N']}")


def _parse_frame(buf, i: int) -> dict:
    try:
        return parse_header(buf)
    except (ValueError, struct.error) as e:
        raise ValueError(f"frame {i}: {e}") from None


class Video:
    """The frames of a container file or of a stream list: ``H``, ``W``,
    ``num_frames``, ``fps`` (numerator, denominator), ``key_frames`` (indices
    from 0), ``frame(i)`` (the stream's bytes), ``span(i)`` (the frames a
    decoder needs for frame i: from the last key frame <= i to i)."""

    def __init__(self, streams: Sequence[bytes], heads: Sequence[dict], fps=(30, 1), file_bytes: int = 0,
                 fmt: Optional[YuvFormat] = None):
        self._streams = streams
        self.format = fmt or YuvFormat()  # the source's pixel format (the header's flags)
        self.H, self.W = int(heads[0]["H"]), int(heads[0]["W"])
        self.num_frames = len(streams)
        self.fps = (int(fps[0]), int(fps[1]))
        self.key_frames = [i for i, h in enumerate(heads) if not h["delta"]]
        self.sizes = [int(h["N"]) for h in heads]
        self.versions = [int(h["version"]) for h in heads]
        self.file_bytes = int(file_bytes)

    def frame(self, i: int) -> bytes:
        if not 0 <= i < self.num_frames:
            raise IndexError(f"frame {i} of {self.num_frames}")
        return self._streams[i]

    def span(self, i: int) -> range:
        if not 0 <= i < self.num_frames:
            raise IndexError(f"frame {i} of {self.num_frames}")
        return range(max(k for k in self.key_frames if k <= i), i + 1)


def _video_of_streams(streams: Sequence[bytes]) -> Video:
    streams = [bytes(s) for s in streams]
    heads = [_parse_frame(s, i) for i, s in enumerate(streams)]
    _check_sequence(heads)
    return Video(streams, heads)


def write_video(path, streams: Sequence[bytes], fps=(30, 1), fmt: Optional[YuvFormat] = None) -> int:
    """Write the frame streams (``encode_frame``, either version) as one file;
    returns its size.  The streams are checked as ``read_video`` will.  ``fmt``:
    the source's pixel format, kept in the header's flags (None: the legacy
    format, flags 0)."""
    vid = _video_of_streams(streams)
    fmt = fmt or YuvFormat()
    flags = fmt.flags
    fps_num, fps_den = int(fps[0]), int(fps[1])
    if fps_num <= 0 or fps_den <= 0:
        raise ValueError("fps is (numerator, denominator), both positive")
    index, off = [], FILE_HEADER_BYTES
    for i in range(vid.num_frames):
        s = vid.frame(i)
        index.append(_INDEX_ENTRY.pack(off, len(s), 0 if i in vid.key_frames else FLAG_DELTA))
        off += len(s)
    index_offset = off
    file_bytes = index_offset + INDEX_ENTRY_BYTES * vid.num_frames
    head = _FILE_HEADER.pack(FILE_MAGIC, FILE_VERSION, vid.H, vid.W, vid.num_frames, fps_num, fps_den, flags,
                             index_offset, file_bytes)
    with open(path, "wb") as fh:
        head += _LAYOUT_WORD.pack(fmt.layout_code)
        fh.write(head + bytes(FILE_HEADER_BYTES - len(head)))
        for i in range(vid.num_frames):
            fh.write(vid.frame(i))
        fh.write(b"".join(index))
    return file_bytes


def read_video(path) -> Video:
    """Open a container file.  Everything is checked here, before anything is
    sized or launched from it (ValueError): magic and version; ``file_bytes``
    against the real size and the index; the index entries ascending, disjoint
    and inside the stream area; each entry's length against its own frame
    header; every frame's size against the file's; frame 0 not a delta; a
    delta's N against its predecessor's."""
    with open(path, "rb") as fh:
        blob = fh.read()
    if len(blob) < FILE_HEADER_BYTES:
        raise ValueError(f"{len(blob)} bytes: shorter than the {FILE_HEADER_BYTES}-byte file header")
    (magic, version, H, W, num_frames, fps_num, fps_den, flags, index_offset,
     file_bytes) = _FILE_HEADER.unpack_from(blob, 0)
    if magic != FILE_MAGIC:
        raise ValueError(f"wrong magic {magic!r}, not {FILE_MAGIC!r}")
    if version != FILE_VERSION:
        raise ValueError(f"file version {version}, not {FILE_VERSION}")
    # ValueError("unknown file flags ...") for an undefined bit, ("unknown layout code ...")
    fmt = YuvFormat.from_flags(flags, _LAYOUT_WORD.unpack_from(blob, _FILE_HEADER.size)[0])
    if any(blob[_FILE_HEADER.size + _LAYOUT_WORD.size:FILE_HEADER_BYTES]):
        raise ValueError("unknown file flags or non-zero reserved header bytes")
    if file_bytes != len(blob):
        raise ValueError(f"file_bytes = {file_bytes}, the file has {len(blob)} (truncated or padded)")
    if num_frames == 0:
        raise ValueError("a video has at least one frame")
    if file_bytes != index_offset + INDEX_ENTRY_BYTES * num_frames:
        raise ValueError(f"file_bytes = {file_bytes}, index_offset = {index_offset} and {num_frames} "
                         f"frames give {index_offset + INDEX_ENTRY_BYTES * num_frames}")
    if index_offset < FILE_HEADER_BYTES:
        raise ValueError(f"index_offset = {index_offset} lies inside the file header")
    if fps_num == 0 or fps_den == 0:
        raise ValueError("fps numerator and denominator must be positive")
    end = FILE_HEADER_BYTES
    entries = []
    for i in range(num_frames):
        off, length, eflags = _INDEX_ENTRY.unpack_from(blob, index_offset + INDEX_ENTRY_BYTES * i)
        if off < end:
            raise ValueError(f"index entry {i}: offset {off} is below {end} (entries ascend and do not "
                             "overlap, after the file header)")
        if length < HEADER_BYTES or off + length > index_offset:
            raise ValueError(f"index entry {i}: [{off}, {off + length}) is no frame inside "
                             f"[{FILE_HEADER_BYTES}, {index_offset})")
        if eflags & ~FLAG_DELTA:
            raise ValueError(f"index entry {i}: unknown flags 0x{eflags:x}")
        end = off + length
        entries.append((off, length, eflags))
    streams, heads = [], []
    for i, (off, length, eflags) in enumerate(entries):
        s = blob[off:off + length]
        h = _parse_frame(s, i)  # the length its own header implies, either version
        if bool(eflags & FLAG_DELTA) != h["delta"]:
            raise ValueError(f"index entry {i}: delta flag differs from the frame header's")
        streams.append(s)
        heads.append(h)
    _check_sequence(heads, H, W)
    return Video(streams, heads, (fps_num, fps_den), file_bytes, fmt)


def _psnr(sse: int, count: int, peak: int = 255) -> float:
    return math.inf if sse == 0 else 10.0 * math.log10(float(peak) * float(peak) * count / sse)


def decode_video(src, out_path=None, device="cuda", batch: int = 8, frames: Optional[range] = None,
                 reference=None, fmt: Optional[YuvFormat] = None, size=None, crop=None, aa=None) -> dict:
    """Decode a container file (a path) or a list of frame streams to YUV
    (planar 4:2:0 unless the format says otherwise), appended frame by frame to ``out_path`` (a raw .yuv; nothing
    is written when None).  ``fmt``: the output's pixel format; None means the
    file's own (``Video.format``: the source's; 8-bit I420, BT.601 limited
    range for a stream list and for files written before the header carried
    one).  Any other value re-targets the output -- the models are float, so
    any depth can be written -- and ``reference`` is read in that format.

    Frames are decoded in batches of at most ``batch``: one
    ``decode_frames(output="i420")`` call each, the decoded parameters of a
    batch's last frame carried into the next, so a batch may begin inside a
    GOP.  On a HIP device each batch is copied into one of two pinned host
    buffers behind its kernels and an event recorded; the host writes the
    batch before it to the file meanwhile.  Two waits: the host waits for a
    buffer's event before it reads it, and a buffer's file write has returned
    before the copy that overwrites it is enqueued (one thread does both).

    ``frames=range(a, b)`` decodes from the key frame of ``span(a)`` and
    discards what precedes ``a``.  ``reference``: the source .yuv; adds
    per-frame ``psnr_y / psnr_u / psnr_v`` (peak 2^bit_depth - 1, from the kernel's
    exact integer SSE, float64 on the host; inf for identical planes) and
    ``psnr_yuv`` = (6 Y + U + V) / 8.  Returns {"frames", "bytes_written",
    "seconds" (host clock, ending in a synchronise), "height", "width" (of the
    frames written), and the PSNR lists}.

    ``size=(H2, W2)`` and ``crop=(x0, y0, w, h)`` decode at another size and
    window (``decode_frames``: the models sampled at the view's positions, no
    prefilter): the frames written, the pinned buffers and ``bytes_written``
    follow H2 x W2, and ``reference`` needs the identity view.  ``aa`` (k,
    (ky, kx) or "auto") adds the box prefilter of ``render.View``: every output
    pixel the mean of ky x kx samples, reduced inside the composite."""
    vid = read_video(src) if isinstance(src, (str, os.PathLike)) else _video_of_streams(src)
    device = torch.device(device)
    batch = int(batch)
    if batch <= 0:
        raise ValueError("batch must be positive")
    a, b = (0, vid.num_frames) if frames is None else (frames.start, frames.stop)
    if frames is not None and frames.step != 1 or not 0 <= a < b <= vid.num_frames:
        raise ValueError(f"frames must be a range(a, b) with 0 <= a < b <= {vid.num_frames}")
    H, W = vid.H, vid.W
    fmt = fmt or vid.format
    view, view_size = None, size  # (``size`` below: a frame's bytes)
    if size is not None or crop is not None or aa is not None:
        from .render import view_of
        view = view_of(H, W, size, crop, aa)
        if reference is not None and not view.is_identity:
            raise ValueError("decode_video: reference frames have the source's size; a view that is not "
                             "the identity cannot be compared with them")
        H, W = view.out_h, view.out_w  # the output's: what is checked, sized and written below
    if fmt.is_planar420 and (H % 2 or W % 2):
        raise ValueError(f"I420 needs an even height and width, not {H}x{W}")
    fmt.check_size(H, W)  # 4:2:2: W even; 4:4:4: any size
    size = fmt.frame_bytes(H, W)
    mm = None
    if reference is not None:
        mm = np.memmap(reference, dtype=np.uint8, mode="r")
        if mm.shape[0] < b * size:
            raise ValueError(f"{reference} holds {mm.shape[0] // size} frames of {W}x{H}, frame "
                             f"{b - 1} is needed")
    cuda = device.type == "cuda"
    pinned = pinned_sse = None
    if cuda:
        pinned = [torch.empty((min(batch, b - a), size), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        pinned_sse = [torch.empty((min(batch, b - a), 3), dtype=torch.int64, pin_memory=True) for _ in range(2)]
        events = [torch.cuda.Event(), torch.cuda.Event()]
    sse_rows: List[np.ndarray] = []
    written = 0
    fh = open(out_path, "wb") if out_path is not None else None

    def flush(item) -> int:
        """Host side of one batch: wait for its copy, write it, keep its SSE."""
        slot, count, host, host_sse = item
        if slot is not None:
            events[slot].synchronize()
        if host_sse is not None:
            sse_rows.append(host_sse[:count].numpy().copy())
        if fh is None:
            return 0
        fh.write(memoryview(host[:count].numpy()).cast("B"))
        return count * size

    try:
        if cuda:
            torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        state, pending, turn = None, None, 0
        for s in range(vid.span(a)[0], b, batch):
            e = min(s + batch, b)
            streams = [vid.frame(i) for i in range(s, e)]
            ref = None
            if mm is not None:
                ref = torch.from_numpy(np.array(mm[s * size:e * size])).to(device)
            if view is None:
                out, state = decode_frames(streams, device, prev=state, return_state=True, output="i420",
                                           reference=ref, fmt=fmt)
            else:
                out, state = decode_frames(streams, device, prev=state, return_state=True, output="i420",
                                           reference=ref, fmt=fmt, size=view_size, crop=crop, aa=aa)
            sse = None
            if ref is not None:
                out, sse = out
            lo = max(a - s, 0)  # frames of this batch before ``a``: decoded for their state only
            count = e - s - lo
            if count <= 0:
                continue
            if cuda:
                slot = turn & 1
                turn += 1
                # pinned[slot] was written to the file two batches ago, in flush() below
                pinned[slot][:count].copy_(out[lo:], non_blocking=True)
                if sse is not None:
                    pinned_sse[slot][:count].copy_(sse[lo:], non_blocking=True)
                events[slot].record(torch.cuda.current_stream(device))
                item = (slot, count, pinned[slot], pinned_sse[slot] if sse is not None else None)
            else:
                item = (None, count, out[lo:], sse[lo:] if sse is not None else None)
            if pending is not None:  # the batch before, while this one runs
                written += flush(pending)
            pending = item
        written += flush(pending)
        if fh is not None:
            fh.flush()
        if cuda:
            torch.cuda.synchronize(device)
        seconds = time.perf_counter() - t0
    finally:
        if fh is not None:
            fh.close()
    res = {"frames": b - a, "bytes_written": written, "seconds": seconds, "height": H, "width": W}
    if mm is not None:
        tot = np.concatenate(sse_rows).astype(np.int64)
        n, cn = H * W, math.prod(fmt.chroma_shape(H, W))
        res["psnr_y"] = [_psnr(int(r[0]), n, fmt.peak) for r in tot]
        res["psnr_u"] = [_psnr(int(r[1]), cn, fmt.peak) for r in tot]
        res["psnr_v"] = [_psnr(int(r[2]), cn, fmt.peak) for r in tot]
        res["psnr_yuv"] = [(6.0 * y + u + v) / 8.0
                           for y, u, v in zip(res["psnr_y"], res["psnr_u"], res["psnr_v"])]
    return res


# --------------------------------------------------------------------------
# command line

def _default_device() -> str:
    return "cuda" if torch.cuda.is_available() else "cpu"


def _info(args) -> dict:
    vid = read_video(args.file)
    streams = sum(len(vid.frame(i)) for i in range(vid.num_frames))
    return {"H": vid.H, "W": vid.W, "frames": vid.num_frames, "fps": list(vid.fps),
            "key_frames": vid.key_frames, "file_bytes": vid.file_bytes,
            "format": {"bit_depth": vid.format.bit_depth, "matrix": vid.format.matrix,
                       "full_range": vid.format.full_range},
            "chroma": vid.format.chroma, "layout": vid.format.layout, "pix_fmt": vid.format.pix_fmt,
            "bpp": round(8.0 * streams / (vid.num_frames * vid.H * vid.W), 6),
            "splats": vid.sizes, "entropy_coded": sum(v == 2 for v in vid.versions)}


def _decode(args) -> dict:
    frames = None
    if args.frames:
        lo, _, hi = args.frames.partition(":")
        frames = range(int(lo or 0), int(hi) if hi else read_video(args.file).num_frames)
    fmt = format_of_arguments(args)  # an override: on top of the file's own format
    if fmt is not None:
        fmt = format_of_arguments(args, read_video(args.file).format)
    size = crop = None
    if args.size:
        try:
            w, h = (int(v) for v in args.size.lower().split("x"))
        except ValueError:
            raise ValueError(f"--size is WxH, not {args.size!r}") from None
        size = (h, w)
    if args.crop:
        try:
            crop = tuple(float(v) for v in args.crop.split(","))
        except ValueError:
            crop = ()
        if len(crop) != 4:
            raise ValueError(f"--crop is X,Y,W,H, not {args.crop!r}")
    aa = None
    if args.aa:
        try:
            k = () if args.aa == "auto" else tuple(int(v) for v in args.aa.lower().split("x"))
        except ValueError:
            k = (0, 0, 0)
        if len(k) > 2:
            raise ValueError(f"--aa is auto, K or KYxKX, not {args.aa!r}")
        aa = "auto" if not k else k[0] if len(k) == 1 else k
    return decode_video(args.file, args.out, device=args.device, batch=args.batch, frames=frames,
                        reference=args.reference, fmt=fmt, size=size, crop=crop, aa=aa)


def _encode(args) -> dict:
    from .compress import compress_video
    from .video import load_yuv_frames, yuv_loss_of_arguments
    state = torch.load(args.models, map_location="cpu")
    count = sum(1 for k in state if k.startswith("frame_"))
    fmt = format_of_arguments(args)
    by_index, total = load_yuv_frames(args.src, args.width, args.height, torch.device(args.device),
                                      range(count), fmt=fmt)
    if total < count:
        raise ValueError(f"{args.models} holds {count} frame models, {args.src} {total} frames")
    k_frames = sorted({1} | {int(x) for x in args.k_frames.split(",") if x.strip()})
    res = compress_video(state, [by_index[i] for i in range(count)], K_frames=k_frames,
                         iterations=args.iterations, lr=args.lr, device=args.device,
                         delta_base=args.delta_base, seed=args.seed, entropy=args.entropy,
                         fused=args.fused, run=args.run_length, loss_type=args.loss_type,
                         yuv_loss=yuv_loss_of_arguments(args))
    size = write_video(args.out, res["streams"], fps=(args.fps_num, args.fps_den), fmt=fmt)
    return {"frames": count, "file_bytes": size, "k_frames": k_frames,
            "bpp": round(8.0 * sum(len(s) for s in res["streams"]) / (count * args.width * args.height), 6),
            "psnr": [round(p, 4) for p in res["psnr"]]}


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(prog="python -m gsvc_amd.codec",
                                 description="GSVC container: encode, inspect, decode to I420")
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("info", help="the header and index of a container file")
    p.add_argument("file")
    p.set_defaults(run=_info)
    p = sub.add_parser("decode", help="container file -> raw planar I420 (.yuv)")
    p.add_argument("file")
    p.add_argument("out")
    p.add_argument("--device", default=_default_device())
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--frames", default=None, help="A:B, frames A <= i < B from 0 (default all)")
    p.add_argument("--reference", default=None, help="the source .yuv, in the output's format: per-frame PSNR")
    p.add_argument("--size", default=None, metavar="WxH",
                   help="the output's size (default the file's): the models sampled at that grid, no prefilter")
    p.add_argument("--crop", default=None, metavar="X,Y,W,H",
                   help="a window of the frame in source pixels, fractions allowed (default the whole frame)")
    p.add_argument("--aa", default=None, metavar="auto|K|KYxKX",
                   help="box prefilter: every output pixel the mean of KY x KX samples (auto: the downscale's "
                        "factor per axis, at most 8)")
    add_format_arguments(p)  # override the file's own format
    p.set_defaults(run=_decode)
    p = sub.add_parser("encode", help="overfit frame models + source .yuv -> container file")
    p.add_argument("models", help="gmodels_state_dict.pth of gsvc_amd.video (frame_<n> from 1)")
    p.add_argument("src", help="the source video, raw YUV (planar 4:2:0 unless --chroma / --layout / --pix_fmt)")
    p.add_argument("out")
    p.add_argument("--width", type=int, required=True)
    p.add_argument("--height", type=int, required=True)
    p.add_argument("--k_frames", default="1", help="comma list of key frames, from 1")
    p.add_argument("--iterations", type=int, default=30000)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--entropy", action="store_true", help="entropy-coded frame streams (version 2)")
    p.add_argument("--fused", action="store_true", help="the one-call training step (HIP devices)")
    p.add_argument("--run", dest="run_length", type=int, default=None, metavar="K",
                   help="with --fused: K iterations per call, the best state kept on the device")
    p.add_argument("--delta_base", choices=["overfit", "decoded"], default="decoded",
                   help="decoded (default): the file decodes to what training measured")
    p.add_argument("--loss_type", default="L2",
                   help="L2 (default), L1, or YUV: the weighted Y/U/V loss in src's colour space and chroma "
                        "(--matrix --full_range --chroma --pix_fmt)")
    p.add_argument("--loss_weights", default=None, metavar="WY,WU,WV",
                   help="plane weights of --loss_type YUV (default 6,1,1)")
    p.add_argument("--fps_num", type=int, default=30)
    p.add_argument("--fps_den", type=int, default=1)
    add_format_arguments(p)  # of src; stored in the file
    p.add_argument("--device", default=_default_device())
    p.set_defaults(run=_encode)
    args = ap.parse_args(argv)
    res = args.run(args)
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
