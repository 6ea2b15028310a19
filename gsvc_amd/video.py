"""GSVC's video driver on the gsvc_amd hot path, sharded by GOP across GPUs.

A restatement of train_video_Represent.py (reference :17-401) and the helpers
it uses from utils.py (process_yuv_video :134-156, EarlyStopping :188-211,
detect_outliers_mean_diff :214-229) that runs on the MI355X path:

* frames come from a planar YUV 4:2:0 file (converted on the GPU: 8-bit I420
  by ``gsvc_i420_to_rgb``, OpenCV's BT.601 arithmetic; 10, 12 and 16 bits,
  BT.709 and full range by ``gsvc_yuv420_to_rgb``, ``--bit_depth --matrix
  --full_range``; 4:2:2, 4:4:4 and semi-planar NV12 / P010 files by
  ``gsvc_yuv_to_rgb``, ``--chroma --layout --pix_fmt``) or from a seeded
  synthetic video (the UVG sequences are not in this image);
* K-frames (key frames, trained from scratch) come from
  ``<savdir>/<data>/K_frames.txt`` when present, else from the reference's
  detector (500 scratch iterations and a 100-iteration P-probe per frame,
  normalised loss differences, mean-difference outliers), run with every
  rank taking a contiguous frame range plus a one-frame halo;
* the frames are split into GOPs (a K-frame and the P-frames after it, which
  start from the previous frame's model) and ranks take contiguous GOPs
  (shard.py); when there are fewer GOPs than ranks, K-frames are forced at
  the shard boundaries; K_frames_used.txt records the GOPs trained and a
  missing K_frames.txt is written from detection (never overwritten);
* each frame trains with ``GaussianVideoFrame.train_iter`` (the fused step on
  the GPU), early stopping as the reference, then PSNR and the eval FPS of
  100 renders (synchronised);
* the per-frame metrics meet in ONE all_reduce (RCCL over xGMI with the
  "nccl" backend; gloo on CPU), the only collective of the path;
* ``--ranks_per_gpu R`` puts R ranks (R GOP shards) on each GPU: one frame's
  step leaves part of the chip idle, so two concurrent shards train ~1.35x as
  many iterations per second; their collectives go over gloo.

    python -m gsvc_amd.video --synthetic 24 --width 256 --height 256 --num_points 2000 \\
        --iterations 300 --loss_type L2
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 -m gsvc_amd.video -d Beauty.yuv ...

The per-frame MS-SSIM is gsvc_amd.msssim.ms_ssim (pytorch_msssim's algorithm
on the gfx950 kernels; parity unpinned against the package);
frames whose smaller side is <= 160 (where ms_ssim asserts) report NaN.
"""
from __future__ import annotations

import argparse
import ctypes
import dataclasses
import json
import math
import os
import time
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from .frame import GaussianVideoFrame
from .msssim import ms_ssim
from .shard import aggregate_video_metrics, forced_k_frames, gops, shard_gops

# ---------------------------------------------------------------------------
# frames


_DEPTHS = (8, 10, 12, 16)       # the container's depth codes 0..3
_MATRICES = ("bt601", "bt709")  # (Kr, Kb) below; the container's matrix bit
_KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
_FLAG_DEPTH, _FLAG_MATRIX, _FLAG_FULL = 0x3, 0x10, 0x40


_CHROMAS = ("420", "422", "444")   # the layout code's bits 0-1
_LAYOUTS = ("planar", "semi")      # the layout code's bit 4
_LAYOUT_CHROMA, _LAYOUT_SEMI = 0x3, 0x10
# the legacy triple's constants (csrc/yuv.hip, csrc/yuv_conv.hip's kLegacyTable:
# OpenCV's three decimals) in gsvc_yuv_format_table's order: what every layout
# computes with at 8-bit bt601 limited range
_LEGACY_TABLE = (255, 16, 128, 1, 1220542, 1673527, -409993, -852492, 2116026, 269484, 528482, 102760,
                 -155188, -305135, 460324, 460324, -385875, -74448)


@dataclasses.dataclass(frozen=True)
class YuvFormat:
    """A YUV pixel format: ``bit_depth`` 8, 10, 12 or 16, ``matrix`` "bt601" or
    "bt709", limited or full range, ``chroma`` "420", "422" or "444", ``layout``
    "planar" (planes Y, U, V) or "semi" (plane Y, then one plane of interleaved
    U, V pairs, U first: NV12 / NV16 / NV24).  Above 8 bits the samples are
    16-bit little-endian words: planar with the value in the low bits
    (yuv420p10le), semi-planar with the value in the high bits (the P010
    family: word = value << (16 - bit_depth)).
    ``YuvFormat()`` is the legacy format (planar 4:2:0, 8-bit BT.601 limited
    range), which keeps OpenCV's constants (csrc/yuv.hip in, csrc/yuv_conv.hip
    out); every other colour triple takes gsvc_yuv_format_table's exact
    coefficients, every chroma and layout the same kernels of
    csrc/yuv_conv.hip."""
    bit_depth: int = 8
    matrix: str = "bt601"
    full_range: bool = False
    chroma: str = "420"
    layout: str = "planar"

    def __post_init__(self):
        if self.bit_depth not in _DEPTHS or isinstance(self.bit_depth, bool):
            raise ValueError(f"bit_depth is one of {_DEPTHS}, not {self.bit_depth!r}")
        if self.matrix not in _MATRICES:
            raise ValueError(f"matrix is one of {_MATRICES}, not {self.matrix!r}")
        chroma = str(self.chroma) if isinstance(self.chroma, int) and not isinstance(self.chroma, bool) \
            else self.chroma
        if chroma not in _CHROMAS:
            raise ValueError(f"chroma is one of {_CHROMAS}, not {self.chroma!r}")
        if self.layout not in _LAYOUTS:
            raise ValueError(f"layout is one of {_LAYOUTS}, not {self.layout!r}")
        object.__setattr__(self, "bit_depth", int(self.bit_depth))
        object.__setattr__(self, "full_range", bool(self.full_range))
        object.__setattr__(self, "chroma", chroma)

    @property
    def peak(self) -> int:
        return (1 << self.bit_depth) - 1

    @property
    def sample_bytes(self) -> int:
        return 1 if self.bit_depth == 8 else 2

    @property
    def is_planar420(self) -> bool:
        """The layout of gsvc_i420_to_rgb / gsvc_rgb_to_i420 and gsvc_yuv420_to_rgb / gsvc_rgb_to_yuv420."""
        return self.chroma == "420" and self.layout == "planar"

    @property
    def msb_shift(self) -> int:
        """Semi-planar words carry the value in the high bits: word = value << msb_shift."""
        return 16 - self.bit_depth if self.layout == "semi" and self.bit_depth > 8 else 0

    def chroma_shape(self, height: int, width: int):
        """(rows, columns) of the U samples (and of the V samples) of an H x W frame."""
        return (height // 2 if self.chroma == "420" else height,
                width if self.chroma == "444" else width // 2)

    def check_size(self, height: int, width: int) -> None:
        """ValueError unless H x W fits the chroma: 4:2:0 both even, 4:2:2 W even."""
        if height <= 0 or width <= 0:
            raise ValueError(f"height and width must be positive, not {height}x{width}")
        if self.chroma == "420" and (height % 2 or width % 2):
            raise ValueError(f"4:2:0 needs an even height and width, not {height}x{width}")
        if self.chroma == "422" and width % 2:
            raise ValueError(f"4:2:2 needs an even width, not {height}x{width}")

    def plane_shapes(self, height: int, width: int):
        """The planes of one frame in file order, as (rows, samples per row):
        planar Y, U, V; semi-planar Y and the interleaved plane."""
        self.check_size(height, width)
        ch, cw = self.chroma_shape(height, width)
        if self.layout == "semi":
            return ((height, width), (ch, 2 * cw))
        return ((height, width), (ch, cw), (ch, cw))

    def frame_bytes(self, height: int, width: int) -> int:
        if self.chroma == "420":
            return height * width * 3 // 2 * self.sample_bytes
        ch, cw = self.chroma_shape(height, width)
        return (height * width + 2 * ch * cw) * self.sample_bytes

    @property
    def is_legacy(self) -> bool:
        return self.bit_depth == 8 and self.matrix == "bt601" and not self.full_range and self.is_planar420

    @property
    def flags(self) -> int:
        """The container's code (codec.py): bits 0-1 depth, bit 4 matrix, bit 6 range."""
        return (_DEPTHS.index(self.bit_depth) | (_FLAG_MATRIX if self.matrix == "bt709" else 0) |
                (_FLAG_FULL if self.full_range else 0))

    @property
    def layout_code(self) -> int:
        """The container's layout word (codec.py): bits 0-1 chroma (0: 420, 1: 422,
        2: 444), bit 4 semi-planar."""
        return _CHROMAS.index(self.chroma) | (_LAYOUT_SEMI if self.layout == "semi" else 0)

    @classmethod
    def from_flags(cls, flags: int, layout_code: int = 0) -> "YuvFormat":
        flags, layout_code = int(flags), int(layout_code)
        if flags & ~(_FLAG_DEPTH | _FLAG_MATRIX | _FLAG_FULL):
            raise ValueError(f"unknown file flags 0x{flags:x}")
        if layout_code & ~(_LAYOUT_CHROMA | _LAYOUT_SEMI) or (layout_code & _LAYOUT_CHROMA) >= len(_CHROMAS):
            raise ValueError(f"unknown layout code 0x{layout_code & 0xffffffff:x}")
        return cls(_DEPTHS[flags & _FLAG_DEPTH], _MATRICES[1 if flags & _FLAG_MATRIX else 0],
                   bool(flags & _FLAG_FULL), _CHROMAS[layout_code & _LAYOUT_CHROMA],
                   _LAYOUTS[1 if layout_code & _LAYOUT_SEMI else 0])

    @property
    def pix_fmt(self) -> str:
        """ffmpeg's name of the depth, chroma and layout (matrix and range are not
        part of it): yuv420p, yuv422p10le, nv12, p010le, p210le, ..."""
        if self.layout == "planar":
            return f"yuv{self.chroma}p" + ("" if self.bit_depth == 8 else f"{self.bit_depth}le")
        if self.bit_depth == 8:
            return {"420": "nv12", "422": "nv16", "444": "nv24"}[self.chroma]
        return f"p{_CHROMAS.index(self.chroma) * 2}{self.bit_depth}le"

    @classmethod
    def from_pix_fmt(cls, name: str, matrix: str = "bt601", full_range: bool = False) -> "YuvFormat":
        for depth in _DEPTHS:
            for chroma in _CHROMAS:
                for layout in _LAYOUTS:
                    fmt = cls(depth, matrix, full_range, chroma, layout)
                    if fmt.pix_fmt == name:
                        return fmt
        raise ValueError(f"unknown pix_fmt {name!r}")

    def table(self):
        """gsvc_yuv_format_table's 18 integers (include/gsvc_amd.h): P, Yoff, Coff,
        bytes per sample, cY cRV cGU cGV cBU, yR yG yB, uR uG uB, vR vG vB."""
        b, P = self.bit_depth, float(self.peak)
        kr, kb = _KR_KB[self.matrix]
        kg = 1.0 - kr - kb
        yspan = P if self.full_range else float(219 << (b - 8))
        cspan = P if self.full_range else float(224 << (b - 8))
        fix = lambda x: int(math.floor(x * 1048576.0 + 0.5))  # noqa: E731
        half = fix(cspan / (2.0 * P))
        return (self.peak, 0 if self.full_range else 16 << (b - 8), 1 << (b - 1), self.sample_bytes,
                fix(P / yspan), fix(2.0 * (1.0 - kr) * P / cspan), fix(-2.0 * kb * (1.0 - kb) / kg * P / cspan),
                fix(-2.0 * kr * (1.0 - kr) / kg * P / cspan), fix(2.0 * (1.0 - kb) * P / cspan),
                fix(kr * yspan / P), fix(kg * yspan / P), fix(kb * yspan / P),
                fix(-kr / (2.0 * (1.0 - kb)) * cspan / P), fix(-kg / (2.0 * (1.0 - kb)) * cspan / P), half,
                half, fix(-kg / (2.0 * (1.0 - kr)) * cspan / P), fix(-kb / (2.0 * (1.0 - kr)) * cspan / P))

    def conversion_table(self):
        """The 18 integers the conversions compute with: ``table()``, but the
        legacy kernels' constants for the legacy colour triple (8-bit bt601
        limited range), in any chroma and layout: one definition per triple."""
        if self.bit_depth == 8 and self.matrix == "bt601" and not self.full_range:
            return _LEGACY_TABLE
        return self.table()

    def _c(self):
        """The format as include/gsvc_amd.h's gsvc_yuv_format (three ints)."""
        return (ctypes.c_int * 3)(self.bit_depth, _MATRICES.index(self.matrix), int(self.full_range))

    def __str__(self):
        s = f"{self.bit_depth}-bit {self.matrix} {'full' if self.full_range else 'limited'} range"
        if self.is_planar420:
            return s
        return f"{s} {self.chroma[0]}:{self.chroma[1]}:{self.chroma[2]} {self.layout}"


def add_format_arguments(parser) -> None:
    """--bit_depth, --matrix, --full_range, --chroma, --layout and --pix_fmt of
    this module's and the codec's command lines."""
    parser.add_argument("--bit_depth", type=int, choices=_DEPTHS, default=None,
                        help="bits per sample of the .yuv (default 8; above 8: 16-bit little-endian)")
    parser.add_argument("--matrix", choices=_MATRICES, default=None, help="default bt601")
    parser.add_argument("--full_range", action="store_true", default=None, help="full-range YUV (default limited)")
    parser.add_argument("--chroma", choices=_CHROMAS, default=None, help="chroma subsampling (default 420)")
    parser.add_argument("--layout", choices=_LAYOUTS, default=None,
                        help="planar (Y, U, V; default) or semi (Y, interleaved UV: NV12 / P010)")
    parser.add_argument("--pix_fmt", default=None, metavar="NAME",
                        help="ffmpeg's name for depth, chroma and layout at once: yuv422p10le, nv12, p010le, ...")


def format_of_arguments(args, base: Optional[YuvFormat] = None) -> Optional[YuvFormat]:
    """The format the options name, on top of ``base`` (None: the legacy
    format); None when no option was given and there is no base.  --pix_fmt
    sets depth, chroma and layout; one of those three beside it with another
    value is a ValueError."""
    depth, chroma, layout = args.bit_depth, getattr(args, "chroma", None), getattr(args, "layout", None)
    name = getattr(args, "pix_fmt", None)
    if name is not None:
        named = YuvFormat.from_pix_fmt(name)
        for opt, given, val in (("--bit_depth", depth, named.bit_depth), ("--chroma", chroma, named.chroma),
                                ("--layout", layout, named.layout)):
            if given is not None and given != val:
                raise ValueError(f"--pix_fmt {name} has {opt} {val}, not {given}")
        depth, chroma, layout = named.bit_depth, named.chroma, named.layout
    given = (depth, args.matrix, args.full_range, chroma, layout)
    if all(g is None for g in given) and base is None:
        return None
    base = base or YuvFormat()
    return YuvFormat(*(getattr(base, f) if g is None else g
                       for f, g in zip(("bit_depth", "matrix", "full_range", "chroma", "layout"), given)))


@dataclasses.dataclass(frozen=True)
class YuvLoss:
    """The weighted Y/U/V training loss (``loss_type="YUV"``):
    with d = clamp(render, 0, 1) - target, e_k = sum_c M[k][c] d_c per pixel,
    Y per pixel and U, V averaged over ``fmt``'s chroma block (2x2 at 4:2:0,
    2x1 at 4:2:2, 1x1 at 4:4:4),

        L = sum_k w_k mse_k / sum_k w_k,    mse_k = mean over blocks of (block mean of e_k)^2,

    so 10 log10(1 / mse_k) is plane k's PSNR before sample rounding, in units
    of the format's full code range.  M is the matrix the output conversion
    computes with, ``fmt.conversion_table()[9:18] / 2**20`` (rows Y, U, V):
    only ``fmt.matrix``, ``fmt.full_range`` and ``fmt.chroma`` matter (the depth
    enters through the table's rounding, the layout not at all).  ``matrix``
    overrides M with an explicit 3x3 (another colour space).  ``weights`` are
    (w_Y, w_U, w_V), non-negative with a positive sum; the default is the
    usual 6:1:1."""
    fmt: YuvFormat = YuvFormat()
    weights: tuple = (6.0, 1.0, 1.0)
    matrix: Optional[tuple] = None

    def __post_init__(self):
        if not isinstance(self.fmt, YuvFormat):
            raise TypeError(f"fmt is a YuvFormat, not {type(self.fmt).__name__}")
        w = tuple(float(x) for x in self.weights)
        if len(w) != 3 or not all(math.isfinite(x) and x >= 0.0 for x in w) or not sum(w) > 0.0:
            raise ValueError(f"weights are three non-negative numbers with a positive sum, not {self.weights!r}")
        object.__setattr__(self, "weights", w)
        if self.matrix is not None:
            m = np.asarray(self.matrix, dtype=np.float64)
            if m.shape != (3, 3) or not np.isfinite(m).all():
                raise ValueError("matrix is a finite 3x3 (rows Y, U, V over R, G, B)")
            object.__setattr__(self, "matrix", tuple(tuple(float(x) for x in row) for row in m))

    @property
    def M(self) -> np.ndarray:
        """The 3x3 RGB -> (Y, U, V) matrix as float64, rows Y, U, V."""
        if self.matrix is not None:
            return np.array(self.matrix, dtype=np.float64)
        return np.array(self.fmt.conversion_table()[9:18], dtype=np.float64).reshape(3, 3) / 1048576.0

    @property
    def chroma_code(self) -> int:
        """0: 4:2:0, 1: 4:2:2, 2: 4:4:4 (the container's chroma codes)."""
        return _CHROMAS.index(self.fmt.chroma)

    def check_size(self, height: int, width: int) -> None:
        self.fmt.check_size(height, width)

    def words(self):
        """include/gsvc_amd.h ``loss_yuv``: M row-major, then the weights, as 12 floats."""
        return (ctypes.c_float * 12)(*self.M.reshape(-1).tolist(), *self.weights)


def parse_loss_weights(text: Optional[str]):
    """``--loss_weights WY,WU,WV`` -> a tuple of three floats (None: 6, 1, 1)."""
    if text is None:
        return (6.0, 1.0, 1.0)
    parts = str(text).split(",")
    if len(parts) != 3:
        raise ValueError(f"--loss_weights takes WY,WU,WV, not {text!r}")
    return tuple(float(p) for p in parts)


def _sample_bytes_of(t: torch.Tensor, fmt: YuvFormat, count: int, what: str) -> torch.Tensor:
    """``t`` (uint8 bytes, or int16 samples of a 16-bit format) as a flat uint8
    tensor of ``count`` bytes."""
    if t.dtype == torch.int16 and fmt.sample_bytes == 2:
        t = t.contiguous().view(torch.uint8)
    if t.dtype != torch.uint8:
        raise RuntimeError(f"{what} must be a uint8 tensor (or int16 samples of a 16-bit format)")
    if t.numel() != count:
        raise ValueError(f"{what} must hold {count} bytes ({fmt}), not {t.numel()}")
    return t.reshape(-1)


def _samples_int64(raw: torch.Tensor, fmt: YuvFormat) -> torch.Tensor:
    """Flat uint8 CPU bytes -> int64 samples (little-endian words above 8 bits)."""
    flat = raw.reshape(-1).to(torch.int64)
    return flat if fmt.sample_bytes == 1 else flat[0::2] | (flat[1::2] << 8)


def _samples_bytes(x: torch.Tensor, fmt: YuvFormat) -> torch.Tensor:
    """int64 samples [F, n] in [0, P] -> uint8 [F, n * sample_bytes], little-endian."""
    if fmt.sample_bytes == 1:
        return x.to(torch.uint8)
    return torch.stack([x & 255, x >> 8], dim=-1).to(torch.uint8).reshape(x.shape[0], -1)


def _split_planes(s: torch.Tensor, h: int, w: int, fmt: YuvFormat):
    """int64 words [F, samples per frame] of any chroma and layout -> values
    Y [F, h, w], U, V [F, ch, cw] (the P010 family's low bits dropped)."""
    s = s >> fmt.msb_shift
    f, n = s.shape[0], h * w
    ch, cw = fmt.chroma_shape(h, w)
    y = s[:, :n].view(f, h, w)
    if fmt.layout == "semi":
        uv = s[:, n:].view(f, ch, cw, 2)
        return y, uv[..., 0], uv[..., 1]
    return y, s[:, n:n + ch * cw].view(f, ch, cw), s[:, n + ch * cw:].view(f, ch, cw)


def _join_planes(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, fmt: YuvFormat) -> torch.Tensor:
    """The inverse of ``_split_planes``: int64 words [F, samples per frame]."""
    f = y.shape[0]
    if fmt.layout == "semi":
        c = [torch.stack([u, v], dim=-1).reshape(f, -1)]
    else:
        c = [u.reshape(f, -1), v.reshape(f, -1)]
    return torch.cat([y.reshape(f, -1)] + c, dim=1) << fmt.msb_shift


def _yuv_to_rgb_torch(raw: torch.Tensor, h: int, w: int, fmt: YuvFormat) -> torch.Tensor:
    """The input arithmetic of csrc/yuv_conv.hip (and, for the legacy format, of
    csrc/yuv.hip) in torch int64 ops (CPU tensors), for one frame."""
    P, yoff, coff, _, cy, crv, cgu, cgv, cbu = fmt.conversion_table()[:9]
    y, u, v = _split_planes(_samples_int64(raw, fmt)[None], h, w, fmt)
    y = (y[0] - yoff).clamp_min(0) * cy + (1 << 19)
    ry, rx = (2 if fmt.chroma == "420" else 1), (1 if fmt.chroma == "444" else 2)
    u, v = ((t[0] - coff).repeat_interleave(ry, 0).repeat_interleave(rx, 1) for t in (u, v))
    rgb = torch.stack([y + crv * v, y + cgv * v + cgu * u, y + cbu * u]) >> 20
    return (rgb.clamp(0, P).to(torch.float32) / torch.tensor(float(P), dtype=torch.float32))[None].contiguous()


def _rgb_to_yuv_torch(images: torch.Tensor, ref: Optional[torch.Tensor], fmt: YuvFormat):
    """csrc/yuv_conv.hip's output arithmetic in torch int64 ops (CPU tensors)."""
    F_, _, H, W = images.shape
    P, yoff, coff = fmt.conversion_table()[:3]
    yr, yg, yb, ur, ug, ub, vr, vg, vb = fmt.conversion_table()[9:]
    c = torch.where(images > 0, images, torch.zeros_like(images))  # NaN, -0 -> 0
    c = torch.where(c < 1, c, torch.ones_like(c))
    q = (c * float(P) + 0.5).to(torch.int64)  # fp32: one rounding per op, then truncation
    R, G, B = q[:, 0], q[:, 1], q[:, 2]
    Y = (yr * R + yg * G + yb * B + ((yoff << 20) + (1 << 19))) >> 20
    ch, cw = fmt.chroma_shape(H, W)
    Rs, Gs, Bs = (t.view(F_, ch, H // ch, cw, W // cw).sum(dim=(2, 4)) for t in (R, G, B))
    sh = 20 + (H // ch).bit_length() + (W // cw).bit_length() - 2  # 20 + log2 of the block's pixels
    U = (ur * Rs + ug * Gs + ub * Bs + ((coff << sh) + (1 << (sh - 1)))) >> sh
    V = (vr * Rs + vg * Gs + vb * Bs + ((coff << sh) + (1 << (sh - 1)))) >> sh
    planes = [t.clamp(0, P) for t in (Y, U, V)]
    out = _samples_bytes(_join_planes(*planes, fmt), fmt)
    if ref is None:
        return out
    rp = _split_planes(_samples_int64(ref, fmt).view(F_, -1), H, W, fmt)
    sse = torch.stack([((a - b) * (a - b)).reshape(F_, -1).sum(1) for a, b in zip(planes, rp)], dim=1)
    return out, sse


def i420_to_rgb(yuv: torch.Tensor, height: int, width: int, fmt: Optional[YuvFormat] = None) -> torch.Tensor:
    """One frame (its raw bytes: a uint8 tensor of ``fmt.frame_bytes(H, W)``; for
    a 16-bit format also an int16 tensor of its samples) -> [1, 3, H, W] float
    RGB in [0, 1] on the tensor's device.  ``fmt`` None or ``YuvFormat()``: 8-bit
    I420 with OpenCV's BT.601 arithmetic (cv2.cvtColor(COLOR_YUV2RGB_I420) +
    ToTensor, ``gsvc_i420_to_rgb``, csrc/yuv.hip); any other planar 4:2:0
    format: ``gsvc_yuv420_to_rgb``; 4:2:2, 4:4:4 and semi-planar frames
    (``fmt.chroma``, ``fmt.layout``; any height at 4:2:2, any size at 4:4:4):
    ``gsvc_yuv_to_rgb`` (both csrc/yuv_conv.hip).  A CPU tensor takes the same
    arithmetic in torch integer ops (the codec's encoder on a host without a
    GPU)."""
    fmt = fmt or YuvFormat()
    if fmt.is_legacy:  # the first entry's checks and wording; the size is the C entry's to refuse
        if yuv.dtype != torch.uint8:
            raise RuntimeError("yuv must be a uint8 tensor")
        if yuv.numel() != height * width * 3 // 2:
            raise ValueError("yuv must hold one I420 frame of H*W*3/2 bytes")
        raw = yuv.reshape(-1)
    else:
        if not fmt.is_planar420:
            fmt.check_size(int(height), int(width))
        elif height <= 0 or width <= 0 or height % 2 or width % 2:
            raise ValueError("i420_to_rgb: height and width positive and even")
        raw = _sample_bytes_of(yuv, fmt, fmt.frame_bytes(height, width), "yuv")
    height, width = int(height), int(width)
    if not raw.is_cuda:
        return _yuv_to_rgb_torch(raw, height, width, fmt)
    from . import _lib as L
    if not raw.is_contiguous() or raw.data_ptr() % fmt.sample_bytes:
        raw = raw.clone()  # a 16-bit view at an odd address
    out = torch.empty((1, 3, height, width), dtype=torch.float32, device=raw.device)
    if fmt.is_legacy:
        L.call("gsvc_i420_to_rgb", L.ptr(raw), height, width, L.ptr(out), L.stream(raw.device))
    elif fmt.is_planar420:
        L.call("gsvc_yuv420_to_rgb", 1, L.ptr(raw), height, width, fmt._c(), L.ptr(out), L.stream(raw.device))
    else:
        L.call("gsvc_yuv_to_rgb", 1, L.ptr(raw), height, width, fmt._c(), int(fmt.chroma),
               int(fmt.layout == "semi"), L.ptr(out), L.stream(raw.device))
    return out


def rgb_to_i420(images: torch.Tensor, ref: Optional[torch.Tensor] = None, fmt: Optional[YuvFormat] = None):
    """Float RGB images [F, 3, H, W] (or [3, H, W]; any values) -> frames as the
    bytes of a .yuv file, uint8 [F, fmt.frame_bytes(H, W)]: per frame Y, then U
    and V of half size each way, chroma from the 2x2 block's sum; the inverse of
    ``i420_to_rgb``.  ``fmt`` None or ``YuvFormat()``: 8-bit I420, BT.601 limited
    range (``gsvc_rgb_to_i420``); any other planar 4:2:0 format:
    ``gsvc_rgb_to_yuv420`` (samples above 8 bits as 16-bit little-endian); 4:2:2,
    4:4:4 and semi-planar output (chroma from the 2x1 block's sum or the pixel
    itself; U, V interleaved; the P010 family's words): ``gsvc_rgb_to_yuv`` (all
    three csrc/yuv_conv.hip).  With ``ref`` (source frames, uint8, the output's
    shape; int16 samples for a 16-bit format) also returns the exact sums of
    squared sample differences, int64 [F, 3] (Y, U, V).  CUDA tensors take the
    kernel, CPU tensors the same arithmetic in torch integer ops; the bytes
    are the same."""
    if images.dim() == 3:
        images = images[None]
    if images.dim() != 4 or images.shape[1] != 3 or not images.is_floating_point():
        raise ValueError("images must be a float tensor [F, 3, H, W] or [3, H, W]")
    fmt = fmt or YuvFormat()
    F_, _, H, W = (int(s) for s in images.shape)
    if not fmt.is_planar420:
        if F_ <= 0:
            raise ValueError("rgb_to_i420: at least one frame")
        fmt.check_size(H, W)
    elif F_ <= 0 or H <= 0 or W <= 0 or H % 2 or W % 2:
        raise ValueError("rgb_to_i420: at least one frame; height and width positive and even")
    size = fmt.frame_bytes(H, W)
    if ref is not None and fmt.is_legacy:  # the first entry's check and wording
        if ref.dtype != torch.uint8 or ref.numel() != F_ * size or ref.device != images.device:
            raise ValueError(f"ref must hold {F_} I420 frames of {size} bytes (uint8) on the images' device")
        ref = ref.reshape(-1)
    elif ref is not None:
        if ref.device != images.device:
            raise ValueError("ref must be on the images' device")
        ref = _sample_bytes_of(ref, fmt, F_ * size, "ref")
    if not images.is_cuda:
        return _rgb_to_yuv_torch(images.detach().float(), ref, fmt)
    from . import _lib as L
    src = images.detach()
    if src.dtype is not torch.float32 or not src.is_contiguous():
        src = src.float().contiguous()
    out = torch.empty((F_, size), dtype=torch.uint8, device=src.device)
    sse = None
    if ref is not None:
        if not ref.is_contiguous() or ref.data_ptr() % fmt.sample_bytes:
            ref = ref.clone()  # a 16-bit view at an odd address
        sse = torch.empty((F_, 3), dtype=torch.int64, device=src.device)
    tail = (L.ptr(out), L.ptr(ref), L.ptr(sse), L.stream(src.device))
    if fmt.is_legacy:
        L.call("gsvc_rgb_to_i420", F_, L.ptr(src), H, W, *tail)
    elif fmt.is_planar420:
        L.call("gsvc_rgb_to_yuv420", F_, L.ptr(src), H, W, fmt._c(), *tail)
    else:
        L.call("gsvc_rgb_to_yuv", F_, L.ptr(src), H, W, fmt._c(), int(fmt.chroma), int(fmt.layout == "semi"), *tail)
    return out if ref is None else (out, sse)


def load_yuv_frames(path: str, width: int, height: int, device, frames: Optional[Sequence[int]] = None,
                    fmt: Optional[YuvFormat] = None):
    """process_yuv_video (utils.py:134-156) for the 0-based frame indices
    ``frames`` (all when None): a memory map, one frame at a time to the GPU.
    ``fmt``: the file's pixel format (None: 8-bit I420, BT.601 limited range)."""
    size = (fmt or YuvFormat()).frame_bytes(height, width)
    total = os.path.getsize(path) // size
    mm = np.memmap(path, dtype=np.uint8, mode="r")
    idx = range(total) if frames is None else frames
    out = {}
    for i in idx:
        if not 0 <= i < total:
            continue
        raw = torch.from_numpy(np.array(mm[i * size:(i + 1) * size])).to(device)
        out[i] = i420_to_rgb(raw, height, width, fmt)
    return out, total


def textured_video(num_frames: int, height: int, width: int, seed: int = 0, cut_every: int = 0,
                   device=None, objects: int = 14):
    """A harder stand-in for the UVG sequences: per scene a
    mid-frequency background (drifting sinusoids up to ~30 cycles across the
    frame) under ``objects`` hard-edged elliptical objects, each with its own
    striped / checkered texture (periods 6-24 px) and colours, moving (2-9 px
    per frame) and turning from frame to frame, drawn back to front; a scene
    cut every ``cut_every`` frames.  Sharp edges, texture and motion keep the
    per-frame models training (the smooth pattern of ``synthetic_video``
    converges in a few hundred iterations).  Computed with torch on ``device``
    (CPU by default); frame(i) -> [1, 3, H, W] in [0, 1]."""
    dev = torch.device(device) if device is not None else torch.device("cpu")
    yy, xx = torch.meshgrid(torch.arange(height, device=dev, dtype=torch.float32),
                            torch.arange(width, device=dev, dtype=torch.float32), indexing="ij")
    diag = float(np.hypot(height, width))

    def frame(i: int) -> torch.Tensor:
        scene = i // cut_every if cut_every else 0
        t = float(i - (scene * cut_every if cut_every else 0))
        rng = np.random.default_rng(seed * 7919 + scene * 104729 + 17)
        img = []
        bg = rng.uniform(0, 1, (3, 4, 5))
        for c in range(3):
            acc = torch.zeros((height, width), device=dev)
            for k in range(4):
                fx, fy, ph, vx, vy = (float(v) for v in bg[c, k])
                acc += torch.sin((60 * fx * xx + 60 * fy * yy) / diag * 3.0 +
                                 6.28 * ph + 0.15 * t * (vx - vy))
            img.append(0.5 + 0.35 * acc / 4)
        img = torch.stack(img)
        for _ in range(objects):
            cx, cy = rng.uniform(0, width), rng.uniform(0, height)
            rx, ry = rng.uniform(40, 260), rng.uniform(40, 260)
            ang, w = rng.uniform(0, np.pi), rng.uniform(-0.03, 0.03)
            vx, vy = rng.uniform(-9, 9), rng.uniform(-6, 6)
            period = rng.uniform(6, 24)
            kind = rng.integers(0, 2)
            c1, c2 = rng.uniform(0, 1, 3), rng.uniform(0, 1, 3)
            ox, oy = cx + vx * t, cy + vy * t
            a = ang + w * t
            ca, sa = float(np.cos(a)), float(np.sin(a))
            u = (xx - ox) * ca + (yy - oy) * sa
            v = -(xx - ox) * sa + (yy - oy) * ca
            inside = (u / rx) ** 2 + (v / ry) ** 2 <= 1.0
            if kind == 0:  # stripes
                pat = (torch.floor(u / period) % 2) == 0
            else:  # checks
                pat = ((torch.floor(u / period) + torch.floor(v / period)) % 2) == 0
            for ch in range(3):
                col = torch.where(pat, torch.tensor(float(c1[ch]), device=dev),
                                  torch.tensor(float(c2[ch]), device=dev))
                img[ch] = torch.where(inside, col, img[ch])
        return img.clamp(0, 1)[None].contiguous()

    return frame


def synthetic_video(num_frames: int, height: int, width: int, seed: int = 0, cut_every: int = 0,
                    device=None):
    """A seeded smooth moving RGB pattern (sum of drifting sinusoids per
    channel), with a scene cut (new pattern) every ``cut_every`` frames: the
    stand-in for the UVG sequences.  Returns a function frame(i) -> [1, 3, H, W]
    in [0, 1] so ranks materialise only their own frames: on the CPU (numpy)
    by default, or computed on ``device`` with torch (a 1080p frame is ~36 M
    sines: ~0.3 s on one host core, microseconds on the GPU; the two agree to
    float32 rounding of sin)."""
    if device is not None and torch.device(device).type != "cpu":
        dev = torch.device(device)
        yy_t, xx_t = torch.meshgrid(torch.linspace(0, 1, height, device=dev),
                                    torch.linspace(0, 1, width, device=dev), indexing="ij")

        def frame_dev(i: int) -> torch.Tensor:
            scene = i // cut_every if cut_every else 0
            rng = np.random.default_rng(seed * 1000003 + scene)
            par = rng.uniform(0, 1, (3, 6, 5)).astype(np.float32)
            t = np.float32(i - (scene * cut_every if cut_every else 0))
            chans = []
            for c in range(3):
                acc = torch.zeros((height, width), device=dev)
                for k in range(6):
                    fx, fy, ph, vx, vy = (float(v) for v in par[c, k])
                    acc += torch.sin(12 * fx * xx_t + 12 * fy * yy_t +
                                     (6.28 * ph + float(0.08 * t * (vx + vy))))
                chans.append(0.5 + 0.5 * acc / 6)
            return torch.stack(chans).clamp(0, 1)[None].contiguous()

        return frame_dev
    yy, xx = np.meshgrid(np.linspace(0, 1, height, dtype=np.float32),
                         np.linspace(0, 1, width, dtype=np.float32), indexing="ij")

    def frame(i: int) -> torch.Tensor:
        scene = i // cut_every if cut_every else 0
        rng = np.random.default_rng(seed * 1000003 + scene)
        par = rng.uniform(0, 1, (3, 6, 5)).astype(np.float32)
        t = np.float32(i - (scene * cut_every if cut_every else 0))
        chans = []
        for c in range(3):
            acc = np.zeros((height, width), np.float32)
            for k in range(6):
                fx, fy, ph, vx, vy = par[c, k]
                acc += np.sin(12 * fx * xx + 12 * fy * yy + 6.28 * ph + 0.08 * t * (vx + vy))
            chans.append(0.5 + 0.5 * acc / 6)
        return torch.from_numpy(np.clip(np.stack(chans), 0, 1)[None].astype(np.float32))

    return frame


# ---------------------------------------------------------------------------
# reference helpers (utils.py:188-229)


class EarlyStopping:
    """The convergence test of train_video_Represent.py:79-96 (reference
    utils.py:188-211): stop once ``patience`` consecutive losses have failed to
    beat the best loss so far by more than ``min_delta``; the first loss only
    sets the best."""

    def __init__(self, patience=100, min_delta=0.0):
        self.patience, self.min_delta = patience, min_delta
        self.best_loss = None
        self.counter = 0

    def __call__(self, current_loss) -> bool:
        stale = self.best_loss is not None and not (self.best_loss - current_loss > self.min_delta)
        if stale:
            self.counter += 1
            return self.counter >= self.patience
        first = self.best_loss is None
        self.best_loss, self.counter = current_loss, 0
        return (not first) and self.patience <= 0


def detect_outliers_mean_diff(values, window_size=10, threshold=3):
    """K-frame candidates of train_video_Represent.py:348-353 (reference
    utils.py:214-229): index i is an outlier when it exceeds the mean of its
    window [i - window_size, i + window_size) (clipped to the sequence) by more
    than ``threshold`` population standard deviations of that window, or is
    more than ``threshold`` times that mean."""
    v = np.asarray(values, dtype=np.float64)
    n = len(v)
    lo = np.maximum(np.arange(n) - window_size, 0)
    hi = np.minimum(np.arange(n) + window_size, n)
    stats = np.array([(np.mean(v[a:b]), np.std(v[a:b])) for a, b in zip(lo, hi)]).reshape(n, 2)
    mean, std = stats[:, 0], stats[:, 1]
    hit = ((v - mean) > threshold * std) | (v > mean * threshold)
    return [int(i) for i in np.flatnonzero(hit)]


# ---------------------------------------------------------------------------
# per-frame trainer (SimpleTrainer2d, train_video_Represent.py:17-202)


class FrameTrainer:
    def __init__(self, image: torch.Tensor, frame_num: int, loss_type: str = "L2",
                 num_points: int = 2000, max_num_points: int = 2000, iterations: int = 30000,
                 lr: float = 1e-3, densification_interval: int = 100, trained_model=None,
                 isdensity=False, isremoval=True, removal_rate=0.25, early_stop=True, yuv_loss=None):
        self.device = image.device
        self.early_stop = early_stop  # False: every frame trains for ``iterations``
        self.gt_image = image
        self.frame_num = frame_num
        self.iterations = iterations
        self.isdensity, self.isremoval = isdensity, isremoval
        self.H, self.W = image.shape[2], image.shape[3]
        self.model = GaussianVideoFrame(
            loss_type=loss_type, yuv_loss=yuv_loss, opt_type="adan", num_points=num_points,
            max_num_points=max_num_points, densification_interval=densification_interval,
            iterations=iterations, H=self.H, W=self.W, BLOCK_H=16, BLOCK_W=16, device=self.device,
            lr=lr, quantize=False, removal_rate=removal_rate, isdensity=isdensity,
            isremoval=isremoval).to(self.device)
        if trained_model is not None:  # :64-69, partial load
            sd = self.model.state_dict()
            sd.update({k: v for k, v in trained_model.items() if k in sd})
            self.model.load_state_dict(sd)

    def _filtered(self):
        sd = self.model.state_dict()
        out = {k: sd[k].detach().clone() for k in ("_xyz", "_cholesky")}
        out["_features_dc"] = self.model.get_features.detach().clone()
        return out

    def pre_train(self):
        """:117-133 (the K-frame detector's probe): no early stopping."""
        self.model.train()
        loss = None
        for it in range(1, int(self.iterations) + 1):
            loss, _ = self.model.pre_train_iter(self.gt_image)
        return self._filtered(), float(loss)

    def train(self):
        """:79-114: train with early stopping, then PSNR and eval FPS."""
        self.model.train()
        t0 = time.time()
        early = EarlyStopping(patience=100, min_delta=1e-9)
        stable = 5000
        loss = None
        it = 0
        for it in range(1, int(self.iterations) + 1):
            loss, psnr = self.model.train_iter(self.gt_image, it)
            if not self.early_stop:
                continue
            lv = float(loss.detach())
            if self.isdensity or self.isremoval:
                stable -= 1
                if stable < 0 and early(lv):
                    break
            elif early(lv):
                break
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        train_time = time.time() - t0
        self.model.eval()
        with torch.no_grad():
            out = self.model()["render"]
            mse = F.mse_loss(out.float(), self.gt_image.float())
            psnr = 10 * math.log10(1.0 / float(mse))
            # :145; ms_ssim needs a smaller side > 160 (the reference asserts):
            # smaller frames report NaN
            ms = float("nan")
            if min(self.H, self.W) > 160 and self.device.type == "cuda":
                ms = float(ms_ssim(out.float(), self.gt_image.float(), data_range=1,
                                   size_average=True))
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            t1 = time.time()
            for _ in range(100):
                self.model()
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            eval_time = (time.time() - t1) / 100
        return dict(psnr=psnr, ms_ssim=ms, training_time=train_time,
                    eval_time=eval_time, eval_fps=1.0 / eval_time,
                    num_gaussians=int(self.model._xyz.shape[0]), loss=float(loss.detach()),
                    iterations=it, model=self._filtered())


# ---------------------------------------------------------------------------
# K-frames and the sharded video loop


def _dist():
    import torch.distributed as dist
    return dist if dist.is_available() and dist.is_initialized() else None


def detect_k_frames(frame_fn, num_frames: int, rank: int, world: int, loss_type: str, lr: float,
                    probe_points=5000, scratch_iters=500, probe_iters=100, seed: int = 1,
                    yuv_loss=None) -> List[int]:
    """train_video_Represent.py:318-355 with frames split over ranks: rank r
    probes a contiguous range and recomputes the scratch model of the frame
    before its range (one-frame halo); the normalised loss list is gathered
    so that every rank finds the same outliers."""
    lo, hi = (num_frames * rank) // world, (num_frames * (rank + 1)) // world
    losses: Dict[int, float] = {}
    prev = None
    ykw = {} if yuv_loss is None else {"yuv_loss": yuv_loss}
    for i in range(max(lo - 1, 0), hi):
        img = frame_fn(i)
        # seeded by frame, not by rank: the halo frame's scratch model is the one
        # its owner trains, and the list does not depend on the world size
        torch.manual_seed(seed + i)
        k = FrameTrainer(img, i + 1, loss_type, probe_points, probe_points, scratch_iters, lr,
                         isdensity=False, isremoval=False, **ykw)
        gm, loss_k = k.pre_train()
        if i >= lo:
            if i == 0:
                losses[i] = 0.0
            else:
                p = FrameTrainer(img, i + 1, loss_type, probe_points, probe_points, probe_iters, lr,
                                 trained_model=prev, isdensity=False, isremoval=False, **ykw)
                _, loss_p = p.pre_train()
                losses[i] = loss_p - loss_k
        prev = gm
    d = _dist()
    if d is not None:
        parts = [None] * world
        d.all_gather_object(parts, losses)
        for part in parts:
            losses.update(part)
    vals = np.array([losses[i] for i in range(num_frames)], np.float64)
    rest = vals[1:]
    if len(rest):
        mn, mx = rest.min(), rest.max()
        span = (mx - mn) if mx > mn else 1.0
        norm = [vals[0]] + [(v - mn) / span for v in rest]
    else:
        norm = [vals[0]]
    ks = [int(x + 1) for x in detect_outliers_mean_diff(norm)]
    return sorted(set([1] + ks))


def train_video(frame_fn, num_frames: int, k_frames: Sequence[int], args, rank: int, world: int,
                device) -> Dict:
    """The per-frame loop of train_video_Represent.py:358-398 over this rank's
    GOPs; returns the video-wide averages (one all_reduce) and this rank's
    per-frame log and models."""
    shards = shard_gops(k_frames, num_frames, world)
    mine = shards[rank]
    per = {k: [] for k in ("psnr", "ms_ssim", "training_time", "eval_time", "eval_fps",
                           "num_gaussians")}
    log, models = [], {}
    # (the spec only with --loss_type YUV: a caller's own trainer class keeps its signature)
    ykw = {"yuv_loss": args.yuv_loss} if getattr(args, "yuv_loss", None) is not None else {}
    for start, end in mine:
        gmodel, npts = None, args.num_points
        for f in range(start, end):  # 1-based frame numbers
            img = frame_fn(f - 1).to(device)
            # seeded by frame: a frame's init is the same on any number of ranks
            torch.manual_seed(int(getattr(args, "seed", 1)) + f)
            if f == start:  # a K-frame: from scratch
                tr = FrameTrainer(img, f, args.loss_type, args.num_points, args.num_points,
                                  args.iterations, args.lr, args.densification_interval,
                                  isdensity=False, isremoval=args.is_rm,
                                  removal_rate=args.removal_rate,
                                  early_stop=not getattr(args, "no_early_stop", False), **ykw)
            else:  # a P-frame: from the previous frame's model
                tr = FrameTrainer(img, f, args.loss_type, npts, args.num_points, args.iterations,
                                  args.lr, args.densification_interval, trained_model=gmodel,
                                  isdensity=args.is_ad, isremoval=False,
                                  removal_rate=args.removal_rate,
                                  early_stop=not getattr(args, "no_early_stop", False), **ykw)
            r = tr.train()
            gmodel, npts = r.pop("model"), r["num_gaussians"]
            models[f"frame_{f}"] = {k: v.cpu() for k, v in gmodel.items()}
            for k in per:
                per[k].append(r[k])
            log.append(dict(frame=f, **{k: r[k] for k in r}))
    avg = aggregate_video_metrics(per, device=device if getattr(args, "backend", "") == "nccl"
                                  else None)
    return dict(average=avg, frames=log, models=models, gops=[list(g) for g in mine])


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="GSVC video representation on MI355X")
    ap.add_argument("-d", "--dataset", type=str, default=None,
                    help="raw .yuv file (planar 4:2:0 unless --chroma / --layout / --pix_fmt say otherwise)")
    add_format_arguments(ap)  # of --dataset
    ap.add_argument("--synthetic", type=int, default=0, help="frames of a synthetic video")
    ap.add_argument("--cut_every", type=int, default=0, help="synthetic scene-cut period")
    ap.add_argument("--synthetic_kind", choices=["smooth", "textured"], default="smooth",
                    help="smooth drifting sinusoids, or textured moving objects (harder)")
    ap.add_argument("--no_early_stop", action="store_true",
                    help="train every frame for --iterations (SURVEY 8d config 4: fixed "
                         "iterations per frame, early stopping off)")
    ap.add_argument("--data_name", type=str, default="Synthetic")
    ap.add_argument("--model_name", type=str, default="GaussianVideo")
    ap.add_argument("--savdir", type=str, default="result")
    ap.add_argument("--savdir_m", type=str, default="models")
    ap.add_argument("--image_length", type=int, default=50)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iterations", type=int, default=30000)
    ap.add_argument("--densification_interval", type=int, default=100)
    ap.add_argument("--num_points", type=int, default=10000)
    ap.add_argument("--loss_type", type=str, default="L2",
                    help="L2, L1, the reference's SSIM / Fusion losses, or YUV: the weighted "
                         "Y/U/V loss with chroma subsampled as --chroma / --pix_fmt say, in the "
                         "colour space of --matrix / --full_range (fused step, like L2 / L1)")
    ap.add_argument("--loss_weights", type=str, default=None, metavar="WY,WU,WV",
                    help="plane weights of --loss_type YUV (default 6,1,1)")
    ap.add_argument("--seed", type=float, default=1)
    ap.add_argument("--removal_rate", type=float, default=0.1)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--is_ad", action="store_true")
    ap.add_argument("--is_rm", action="store_true")
    ap.add_argument("--k_frames", type=str, default="auto",
                    help="auto (K_frames.txt, else detect), forced (shard boundaries only), "
                         "or a comma list")
    ap.add_argument("--root", type=str, default="./checkpoints")
    ap.add_argument("--ranks_per_gpu", type=int, default=1,
                    help="ranks sharing one GPU (each trains its own GOPs on its own stream; "
                         "> 1 uses gloo for the metric collectives, RCCL takes one rank per GPU)")
    args = ap.parse_args(argv)
    args.yuv_loss = yuv_loss_of_arguments(args, ap)
    return args


def yuv_loss_of_arguments(args, parser=None):
    """The YuvLoss of --loss_type YUV, --loss_weights and the format options
    (None for another loss type); a bad combination is a usage error."""
    try:
        if args.loss_type != "YUV":
            if getattr(args, "loss_weights", None) is not None:
                raise ValueError("--loss_weights goes with --loss_type YUV")
            return None
        return YuvLoss(format_of_arguments(args) or YuvFormat(), parse_loss_weights(args.loss_weights))
    except ValueError as e:
        if parser is None:
            raise
        parser.error(str(e))


def rank_device(local: int, ranks_per_gpu: int, use_cuda: bool):
    """(device, backend) of a rank: GPU local // ranks_per_gpu.  Frames and
    GOPs are independent, and one frame's training step is a latency chain
    that leaves most of the GPU idle, so several ranks per GPU overlap their
    steps; their only collectives are the metric aggregate and the K-frame
    detector's gathers, so gloo (host) serves them when ranks share a GPU."""
    rpg = max(1, int(ranks_per_gpu))
    if not use_cuda:
        return torch.device("cpu"), "gloo"
    return torch.device("cuda", local // rpg), ("nccl" if rpg == 1 else "gloo")


def main(argv=None):
    args = parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    use_cuda = torch.cuda.is_available()
    device, args.backend = rank_device(local, args.ranks_per_gpu, use_cuda)
    if use_cuda:
        torch.cuda.set_device(device)
    if world > 1:
        import torch.distributed as dist
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group("gloo")
    if args.seed is not None:
        np.random.seed(int(args.seed))

    if args.dataset:
        fmt = format_of_arguments(args)
        size = (fmt or YuvFormat()).frame_bytes(args.height, args.width)
        total = os.path.getsize(args.dataset) // size
        num_frames = min(args.image_length, total)

        def frame_fn(i, _cache={}):
            if i not in _cache:
                _cache.clear()
                fr, _ = load_yuv_frames(args.dataset, args.width, args.height, device, [i], fmt=fmt)
                _cache.update(fr)
            return _cache[i]
    else:
        num_frames = args.synthetic or args.image_length
        make = textured_video if getattr(args, "synthetic_kind", "smooth") == "textured" else synthetic_video
        gen = make(num_frames, args.height, args.width, int(args.seed), args.cut_every, device=device)

        def frame_fn(i):
            return gen(i).to(device)

    base = Path(args.root) / args.savdir / args.data_name
    kfile = base / "K_frames.txt"
    had_kfile = kfile.exists()
    if args.k_frames == "forced":
        k_frames, source = [1], "forced"
    elif args.k_frames not in ("auto",):
        k_frames, source = sorted({1} | {int(x) for x in args.k_frames.split(",") if x.strip()}), "list"
    elif had_kfile:  # the reference's cache (train_video_Represent.py:312-316)
        k_frames, source = [int(x) for x in kfile.read_text().split()], "file"
    else:
        k_frames, source = detect_k_frames(frame_fn, num_frames, rank, world, args.loss_type,
                                           args.lr, seed=int(args.seed),
                                           **({} if args.yuv_loss is None else {"yuv_loss": args.yuv_loss})
                                           ), "detected"
    # too few GOPs for the ranks: K-frames forced at equal-frame shard
    # boundaries
    if len(gops(k_frames, num_frames)) < world:
        k_frames = sorted(set(k_frames) | set(forced_k_frames(num_frames, world)))
    if rank == 0:
        base.mkdir(parents=True, exist_ok=True)
        # the GOPs this run trained; K_frames.txt (which the reference reads) is
        # written only when it did not exist and the list came from detection,
        # so a reference run on the same directory trains the same GOPs --
        # never overwritten
        (base / "K_frames_used.txt").write_text("".join(f"{k}\n" for k in k_frames))
        if not had_kfile and source == "detected":
            kfile.write_text("".join(f"{k}\n" for k in k_frames))

    t0 = time.time()
    res = train_video(frame_fn, num_frames, k_frames, args, rank, world, device)
    wall = time.time() - t0
    out_dir = base / f"{args.model_name}_{args.iterations}_{args.num_points}"
    out_dir.mkdir(parents=True, exist_ok=True)
    mdir = Path(args.root) / args.savdir_m / args.data_name / f"{args.model_name}_{args.iterations}_{args.num_points}"
    mdir.mkdir(parents=True, exist_ok=True)
    # one gmodels_state_dict.pth keyed frame_<n> (train_video_Represent.py:379,384):
    # rank 0 gathers every rank's frames
    models = res["models"]
    d = _dist()
    if d is not None:
        parts = [None] * world if rank == 0 else None
        d.gather_object(models, parts, dst=0)
        if rank == 0:
            models = {}
            for part in parts:
                models.update(part)
    if rank == 0:
        order = sorted(models, key=lambda k: int(k.split("_")[1]))
        torch.save({k: models[k] for k in order}, mdir / "gmodels_state_dict.pth")
    with open(out_dir / f"train_rank{rank}.jsonl", "w") as fh:
        for r in res["frames"]:
            fh.write(json.dumps(r) + "\n")
    if rank == 0:
        avg = res["average"]
        line = dict(frames=avg["frames"], ranks=world, wall_s=wall, k_frames=k_frames,
                    avg_psnr=avg["psnr"], avg_ms_ssim=avg["ms_ssim"],
                    avg_training_time=avg["training_time"], avg_eval_time=avg["eval_time"],
                    avg_eval_fps=avg["eval_fps"], avg_gaussians=avg["num_gaussians"])
        with open(out_dir / "train.txt", "a") as fh:
            fh.write(json.dumps(line) + "\n")
        print(json.dumps(line), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    return res


if __name__ == "__main__":
    main()
