"""The numpy statement of gsvc_rgb_to_i420's arithmetic (float32 ops in the
stated order, int64 afterwards) and the shapes and value classes its tests
share.  Imports nothing from the package."""
import numpy as np

F32 = np.float32

# (H, W): 2x2; 2x6 (V plane at an odd offset, frames at 18-byte steps); 6x10;
# 4x8 (the smallest vector shape); 2x16; 18x24; 16x520 (more than one wave per
# row pair, plus a remainder); 34x258 (bytewise, W % 8 = 2)
SHAPES = [(2, 2), (2, 6), (6, 10), (4, 8), (2, 16), (18, 24), (16, 520), (34, 258)]
FRAMES = [1, 3]
CLASSES = ["uniform", "grid", "ties", "special"]


def quantize(x):
    """min(max(x, 0), 1) * 255 + 0.5, one float32 rounding per op, truncated
    (NaN -> 0 as fmaxf; +inf -> 255, -inf -> 0)."""
    x = np.asarray(x, F32)
    c = np.fmin(np.fmax(x, F32(0)), F32(1)).astype(F32)
    t = (c * F32(255)).astype(F32)
    t = (t + F32(0.5)).astype(F32)
    return t.astype(np.int64)


def luma(r, g, b):
    return (269484 * r + 528482 * g + 102760 * b + (16 << 20) + (1 << 19)) >> 20


def chroma(rs, gs, bs):
    u = (-155188 * rs - 305135 * gs + 460324 * bs + (128 << 22) + (1 << 21)) >> 22
    v = (460324 * rs - 385875 * gs - 74448 * bs + (128 << 22) + (1 << 21)) >> 22
    return u, v


def rgb_to_i420(rgb):
    """[F, 3, H, W] float -> uint8 [F, H*W*3/2]."""
    rgb = np.asarray(rgb, F32)
    f, _, h, w = rgb.shape
    q = quantize(rgb)
    y = luma(q[:, 0], q[:, 1], q[:, 2])
    s = q.reshape(f, 3, h // 2, 2, w // 2, 2).sum(axis=(3, 5))
    u, v = chroma(s[:, 0], s[:, 1], s[:, 2])
    planes = [np.clip(p, 0, 255).astype(np.uint8).reshape(f, -1) for p in (y, u, v)]
    return np.concatenate(planes, axis=1)


def sse(out, ref, h, w):
    """Exact integer sums of squared byte differences, int64 [F, 3] (Y, U, V)."""
    d = out.astype(np.int64) - ref.astype(np.int64)
    d = d * d
    n, cn = h * w, h * w // 4
    return np.stack([d[:, :n].sum(1), d[:, n:n + cn].sum(1), d[:, n + cn:].sum(1)], axis=1)


def psnr(sse_value, count):
    return np.inf if sse_value == 0 else 10.0 * np.log10(255.0 * 255.0 * count / float(sse_value))


def values(kind, f, h, w, seed=0):
    """One value class as float32 [f, 3, h, w]."""
    rng = np.random.default_rng(seed * 1000 + h * 7 + w)
    shape = (f, 3, h, w)
    if kind == "uniform":  # U(-0.25, 1.25): both clamps
        return rng.uniform(-0.25, 1.25, shape).astype(F32)
    k = rng.integers(0, 256, shape)
    if kind == "grid":  # the exact grid k / 255, i420_to_rgb's outputs
        return (k.astype(F32) / F32(255)).astype(F32)
    if kind == "ties":  # the float32 neighbours of (k + 1/2) / 255, one ulp on either side
        t = ((k.astype(np.float64) + 0.5) / 255.0).astype(F32)
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


def reference_frames(f, h, w, seed=0):
    """Random I420 frames, uint8 [f, h*w*3/2]."""
    rng = np.random.default_rng(seed * 77 + h * 3 + w)
    return rng.integers(0, 256, (f, h * w * 3 // 2)).astype(np.uint8)
