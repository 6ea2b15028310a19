"""The numpy statement of csrc/yuv_conv.hip's arithmetic (include/gsvc_amd.h:
float32 ops in the stated order, int64 afterwards), and the formats, shapes and
value classes its tests share.  Imports nothing from the package."""
import math

import numpy as np

from yuv_cases import CLASSES, FRAMES, SHAPES  # noqa: F401  (the same shapes and output classes)

F32 = np.float32
DEPTHS = (8, 10, 12, 16)
MATRICES = ("bt601", "bt709")
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}

# (bit_depth, matrix, full_range)
LEGACY = (8, "bt601", False)
ALL_FORMATS = [(b, m, r) for b in DEPTHS for m in MATRICES for r in (False, True)]
FORMATS = [f for f in ALL_FORMATS if f != LEGACY]  # the 15 the new entries convert
GPU_FORMATS = [(10, "bt709", False), (10, "bt601", False), (10, "bt709", True), (12, "bt709", False),
               (16, "bt709", True), (8, "bt709", False), (8, "bt601", True)]
INPUT_CLASSES = ["legal", "garbage", "low_luma", "chroma_ends"]


def fmt_id(fmt):
    return f"{fmt[0]}-{fmt[1]}-{'full' if fmt[2] else 'limited'}"


def flags(fmt):
    """The container's code: bits 0-1 depth, bit 4 matrix, bit 6 full range."""
    return DEPTHS.index(fmt[0]) | (0x10 if fmt[1] == "bt709" else 0) | (0x40 if fmt[2] else 0)


def spans(fmt):
    """P, Yoff, Coff, Yspan, Cspan."""
    b, _, full = fmt
    P = (1 << b) - 1
    if full:
        return P, 0, 1 << (b - 1), P, P
    return P, 16 << (b - 8), 1 << (b - 1), 219 << (b - 8), 224 << (b - 8)


def real_coefficients(fmt):
    """The 14 coefficients before fix(), as floats, in the table's order."""
    P, _, _, ys, cs = (float(v) for v in spans(fmt))
    kr, kb = KR_KB[fmt[1]]
    kg = 1.0 - kr - kb
    return [P / ys, 2 * (1 - kr) * P / cs, -2 * kb * (1 - kb) / kg * P / cs, -2 * kr * (1 - kr) / kg * P / cs,
            2 * (1 - kb) * P / cs,
            kr * ys / P, kg * ys / P, kb * ys / P,
            -kr / (2 * (1 - kb)) * cs / P, -kg / (2 * (1 - kb)) * cs / P, cs / (2 * P),
            cs / (2 * P), -kg / (2 * (1 - kr)) * cs / P, -kb / (2 * (1 - kr)) * cs / P]


def fix(x):
    return int(math.floor(x * 2.0 ** 20 + 0.5))


def table(fmt):
    """gsvc_yuv_format_table: P, Yoff, Coff, bytes per sample, the 14 coefficients."""
    P, yoff, coff, _, _ = spans(fmt)
    return [P, yoff, coff, 1 if fmt[0] == 8 else 2] + [fix(c) for c in real_coefficients(fmt)]


def sample_dtype(fmt):
    return np.dtype(np.uint8) if fmt[0] == 8 else np.dtype("<u2")


def frame_bytes(fmt, h, w):
    return h * w * 3 // 2 * sample_dtype(fmt).itemsize


def to_bytes(samples, fmt):
    """Samples [F, n] -> the file's bytes, uint8 [F, n * sample_bytes]."""
    s = np.ascontiguousarray(np.asarray(samples).astype(sample_dtype(fmt)))
    return s.view(np.uint8).reshape(s.shape[0], -1)


def from_bytes(raw, fmt):
    """uint8 [F, bytes] -> int64 samples [F, n]."""
    raw = np.ascontiguousarray(raw, np.uint8)
    return raw.view(sample_dtype(fmt)).astype(np.int64).reshape(raw.shape[0], -1)


# ---------------------------------------------------------------------------
# input: samples -> float RGB

def yuv420_to_rgb_int(samples, h, w, fmt, clamp=True):
    """int64 samples [F, h*w*3/2] -> int64 [F, 3, h, w] levels (clamped to [0, P]
    unless ``clamp`` is False: what the clamp would cut)."""
    P, yoff, coff, _, cy, crv, cgu, cgv, cbu = table(fmt)[:9]
    s = np.asarray(samples, np.int64)
    f, n, cn = s.shape[0], h * w, (h // 2) * (w // 2)
    y = np.maximum(s[:, :n].reshape(f, h, w) - yoff, 0) * cy + (1 << 19)
    u, v = ((s[:, n + k * cn:n + (k + 1) * cn].reshape(f, h // 2, w // 2) - coff).repeat(2, 1).repeat(2, 2)
            for k in (0, 1))
    rgb = np.stack([y + crv * v, y + cgv * v + cgu * u, y + cbu * u], axis=1) >> 20
    return np.clip(rgb, 0, P) if clamp else rgb


def yuv420_to_rgb(samples, h, w, fmt):
    """float32 [F, 3, h, w]: (float)X / (float)P, one IEEE division."""
    return (yuv420_to_rgb_int(samples, h, w, fmt).astype(F32) / F32(table(fmt)[0])).astype(F32)


def input_values(kind, f, h, w, fmt, seed=0):
    """One input class as int64 samples [f, h*w*3/2] (each fits the format's sample type)."""
    P, yoff, coff, ys, cs = spans(fmt)
    rng = np.random.default_rng(seed * 911 + h * 5 + w + fmt[0])
    n, cn = h * w, (h // 2) * (w // 2)
    top = 255 if fmt[0] == 8 else 65535
    clo, chi = (0, P) if fmt[2] else (coff - cs // 2, coff + cs // 2)
    y = rng.integers(yoff, yoff + ys + 1, (f, n))
    c = rng.integers(clo, chi + 1, (f, 2 * cn))
    if kind == "legal":  # uniform legal codes
        pass
    elif kind == "garbage":  # every bit pattern of the sample word, above P for b < 16
        y, c = rng.integers(0, top + 1, (f, n)), rng.integers(0, top + 1, (f, 2 * cn))
    elif kind == "low_luma":  # Y below Yoff (all of [0, Yoff]; at full range Y = 0)
        y = rng.integers(0, yoff + 1, (f, n))
    elif kind == "chroma_ends":  # chroma at 0 and P
        c = np.where(rng.integers(0, 2, (f, 2 * cn)) == 0, 0, P)
    else:
        raise ValueError(kind)
    return np.concatenate([y, c], axis=1).astype(np.int64)


# ---------------------------------------------------------------------------
# output: float RGB -> samples

def quantize(x, P):
    """min(max(x, 0), 1) * P + 0.5, one float32 rounding per op, truncated
    (NaN -> 0 as fmaxf; +inf -> P, -inf -> 0)."""
    x = np.asarray(x, F32)
    c = np.fmin(np.fmax(x, F32(0)), F32(1)).astype(F32)
    t = (c * F32(P)).astype(F32)
    t = (t + F32(0.5)).astype(F32)
    return t.astype(np.int64)


def levels_to_yuv(q, fmt):
    """int64 levels [F, 3, h, w] -> int64 samples [F, h*w*3/2]."""
    P, yoff, coff = table(fmt)[:3]
    yr, yg, yb, ur, ug, ub, vr, vg, vb = table(fmt)[9:]
    f, _, h, w = q.shape
    y = (yr * q[:, 0] + yg * q[:, 1] + yb * q[:, 2] + (yoff << 20) + (1 << 19)) >> 20
    s = q.reshape(f, 3, h // 2, 2, w // 2, 2).sum(axis=(3, 5))
    u = (ur * s[:, 0] + ug * s[:, 1] + ub * s[:, 2] + (coff << 22) + (1 << 21)) >> 22
    v = (vr * s[:, 0] + vg * s[:, 1] + vb * s[:, 2] + (coff << 22) + (1 << 21)) >> 22
    return np.concatenate([np.clip(p, 0, P).reshape(f, -1) for p in (y, u, v)], axis=1)


def rgb_to_yuv420(rgb, fmt):
    """[F, 3, H, W] float -> int64 samples [F, H*W*3/2]."""
    return levels_to_yuv(quantize(np.asarray(rgb, F32), table(fmt)[0]), fmt)


def sse(out, ref, h, w):
    """Exact sums of squared sample differences, int64 [F, 3] (Y, U, V); samples as int64."""
    d = np.asarray(out, np.int64) - np.asarray(ref, np.int64)
    d = d * d
    n, cn = h * w, h * w // 4
    return np.stack([d[:, :n].sum(1), d[:, n:n + cn].sum(1), d[:, n + cn:].sum(1)], axis=1)


def psnr(sse_value, count, P):
    return np.inf if sse_value == 0 else 10.0 * np.log10(float(P) * float(P) * count / float(sse_value))


def values(kind, f, h, w, P, seed=0):
    """One output value class as float32 [f, 3, h, w] (tests/yuv_cases.py's, on the grid of P)."""
    rng = np.random.default_rng(seed * 1000 + h * 7 + w + P)
    shape = (f, 3, h, w)
    if kind == "uniform":  # U(-0.25, 1.25): both clamps
        return rng.uniform(-0.25, 1.25, shape).astype(F32)
    k = rng.integers(0, P + 1, shape)
    if kind == "grid":  # the exact grid k / P, the input conversion's outputs
        return (k.astype(F32) / F32(P)).astype(F32)
    if kind == "ties":  # the float32 neighbours of (k + 1/2) / P, one ulp on either side
        t = ((k.astype(np.float64) + 0.5) / float(P)).astype(F32)
        side = rng.integers(0, 3, shape)  # below, the rounded midpoint itself, above
        return np.select([side == 0, side == 1], [np.nextafter(t, F32(-1)), t],
                         np.nextafter(t, F32(2))).astype(F32)
    if kind == "special":  # NaN, +-inf and -0 among ordinary values
        x = rng.uniform(0, 1, shape).astype(F32)
        pick = rng.integers(0, 8, shape)
        x[pick == 0] = np.nan
        x[pick == 1] = np.inf
        x[pick == 2] = -np.inf
        x[pick == 3] = F32(-0.0)
        return x
    raise ValueError(kind)


def reference_samples(f, h, w, fmt, seed=0):
    """Random source frames, int64 samples [f, h*w*3/2] over the whole sample word."""
    rng = np.random.default_rng(seed * 77 + h * 3 + w + fmt[0])
    return rng.integers(0, 256 if fmt[0] == 8 else 65536, (f, h * w * 3 // 2)).astype(np.int64)
