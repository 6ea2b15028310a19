"""The numpy statement of csrc/yuv_conv.hip's arithmetic (DESIGN.md §13f:
yuv_format_cases' formulas with the chroma block generalised to 2x2, 2x1 and
1x1, planar and semi-planar frames, the P010 family's words), and the layouts,
shapes and value classes its tests share.  A layout is (chroma, layout) with
chroma "420" / "422" / "444" and layout "planar" / "semi"; a format is a colour
triple of yuv_format_cases.  Imports nothing from the package."""
import numpy as np

import yuv_cases as Y
import yuv_format_cases as YF

F32 = np.float32
CHROMAS = ("420", "422", "444")
LAYOUTS = ("planar", "semi")
ALL_LAYOUTS = [(c, l) for c in CHROMAS for l in LAYOUTS]
PLANAR420 = ("420", "planar")
NEW_LAYOUTS = [lay for lay in ALL_LAYOUTS if lay != PLANAR420]  # the five the new entries convert
GPU_FORMATS = [(10, "bt709", False), YF.LEGACY, (16, "bt709", True), (12, "bt601", False)]
FRAMES = [1, 3]
# (H, W): the smallest block of each chroma (2x2, 1x2, 1x1); 3x5 (4:4:4, both
# odd); 3x6 (4:2:2, odd H); 6x10 (fallback, W % 8 != 0); 4x8 (one vector unit per
# row); 18x24 (three per row; frames no multiple of 16 bytes); 16x520 (a row
# past one 256-lane block's units)
SHAPES = [(2, 2), (1, 2), (1, 1), (3, 5), (3, 6), (6, 10), (4, 8), (18, 24), (16, 520)]

# the legacy kernels' constants (csrc/yuv.hip, csrc/yuv_conv.hip) in
# gsvc_yuv_format_table's order: the legacy triple's table in every layout
LEGACY_TABLE = [255, 16, 128, 1, 1220542, 1673527, -409993, -852492, 2116026, 269484, 528482, 102760,
                -155188, -305135, 460324, 460324, -385875, -74448]

PIX_FMTS = {  # (depth, chroma, layout) -> ffmpeg's name
    **{(b, c, "planar"): f"yuv{c}p" + ("" if b == 8 else f"{b}le") for b in YF.DEPTHS for c in CHROMAS},
    (8, "420", "semi"): "nv12", (8, "422", "semi"): "nv16", (8, "444", "semi"): "nv24",
    (10, "420", "semi"): "p010le", (12, "420", "semi"): "p012le", (16, "420", "semi"): "p016le",
    (10, "422", "semi"): "p210le", (12, "422", "semi"): "p212le", (16, "422", "semi"): "p216le",
    (10, "444", "semi"): "p410le", (12, "444", "semi"): "p412le", (16, "444", "semi"): "p416le",
}


def lay_id(lay):
    return f"{lay[0]}-{lay[1]}"


def layout_code(lay):
    """The container's layout word: bits 0-1 chroma, bit 4 semi-planar."""
    return CHROMAS.index(lay[0]) | (0x10 if lay[1] == "semi" else 0)


def table(fmt):
    """The 18 integers the conversions of the new layouts compute with."""
    return list(LEGACY_TABLE) if tuple(fmt) == YF.LEGACY else YF.table(fmt)


def block(lay):
    """(rows, columns) of the pixels one chroma sample serves."""
    return (2 if lay[0] == "420" else 1), (1 if lay[0] == "444" else 2)


def fits(lay, h, w):
    by, bx = block(lay)
    return h > 0 and w > 0 and h % by == 0 and w % bx == 0


def chroma_shape(lay, h, w):
    by, bx = block(lay)
    return h // by, w // bx


def plane_shapes(lay, h, w):
    ch, cw = chroma_shape(lay, h, w)
    return ((h, w), (ch, 2 * cw)) if lay[1] == "semi" else ((h, w), (ch, cw), (ch, cw))


def frame_samples(lay, h, w):
    ch, cw = chroma_shape(lay, h, w)
    return h * w + 2 * ch * cw


def frame_bytes(fmt, lay, h, w):
    return frame_samples(lay, h, w) * YF.sample_dtype(fmt).itemsize


def msb_shift(fmt, lay):
    """The P010 family: a semi-planar word above 8 bits is value << (16 - b)."""
    return 16 - fmt[0] if lay[1] == "semi" and fmt[0] > 8 else 0


# ---------------------------------------------------------------------------
# planes <-> words

def join(y, u, v, fmt, lay):
    """Values Y [F, h, w], U, V [F, ch, cw] -> the frame's words, int64 [F, n]."""
    f = y.shape[0]
    if lay[1] == "semi":
        c = [np.stack([u, v], axis=-1).reshape(f, -1)]
    else:
        c = [u.reshape(f, -1), v.reshape(f, -1)]
    return np.concatenate([y.reshape(f, -1)] + c, axis=1).astype(np.int64) << msb_shift(fmt, lay)


def split(words, h, w, fmt, lay):
    """The frame's words [F, n] -> values Y [F, h, w], U, V [F, ch, cw] (the low
    bits of the P010 family's words ignored)."""
    s = np.asarray(words, np.int64) >> msb_shift(fmt, lay)
    f, n = s.shape[0], h * w
    ch, cw = chroma_shape(lay, h, w)
    y = s[:, :n].reshape(f, h, w)
    if lay[1] == "semi":
        uv = s[:, n:].reshape(f, ch, cw, 2)
        return y, uv[..., 0], uv[..., 1]
    return y, s[:, n:n + ch * cw].reshape(f, ch, cw), s[:, n + ch * cw:].reshape(f, ch, cw)


def to_bytes(words, fmt):
    return YF.to_bytes(words, fmt)


def from_bytes(raw, fmt):
    return YF.from_bytes(raw, fmt)


def i420_to_layout(words420, h, w, fmt, lay):
    """A planar 4:2:0 frame's VALUES [F, h*w*3/2] re-laid as ``lay`` (4:2:0 only:
    the permutation nv12 is of I420, and the P010 shift)."""
    assert lay[0] == "420"
    y, u, v = split(words420, h, w, (fmt[0], fmt[1], fmt[2]), PLANAR420)
    return join(y, u, v, fmt, lay)


# ---------------------------------------------------------------------------
# input: words -> float RGB

def yuv_to_rgb_int(words, h, w, fmt, lay, clamp=True):
    P, yoff, coff, _, cy, crv, cgu, cgv, cbu = table(fmt)[:9]
    ys, us, vs = split(words, h, w, fmt, lay)
    by, bx = block(lay)
    y = np.maximum(ys - yoff, 0) * cy + (1 << 19)
    u, v = ((t - coff).repeat(by, 1).repeat(bx, 2) for t in (us, vs))
    rgb = np.stack([y + crv * v, y + cgv * v + cgu * u, y + cbu * u], axis=1) >> 20
    return np.clip(rgb, 0, P) if clamp else rgb


def yuv_to_rgb(words, h, w, fmt, lay):
    """float32 [F, 3, h, w]: (float)X / (float)P, one IEEE division."""
    return (yuv_to_rgb_int(words, h, w, fmt, lay).astype(F32) / F32(table(fmt)[0])).astype(F32)


def input_values(kind, f, h, w, fmt, lay, seed=0):
    """yuv_format_cases' input classes as the frame's words; "low_bits": legal
    values with random bits below the value in the P010 family's words."""
    P, yoff, coff, ys, cs = YF.spans(fmt)
    rng = np.random.default_rng(seed * 911 + h * 5 + w + fmt[0] + 13 * layout_code(lay))
    ch, cw = chroma_shape(lay, h, w)
    top = 255 if fmt[0] == 8 else 65535
    clo, chi = (0, P) if fmt[2] else (coff - cs // 2, coff + cs // 2)
    y = rng.integers(yoff, yoff + ys + 1, (f, h, w))
    c = rng.integers(clo, chi + 1, (2, f, ch, cw))
    sh = msb_shift(fmt, lay)
    if kind == "garbage":  # every bit pattern of the sample word
        n = frame_samples(lay, h, w)
        return rng.integers(0, top + 1, (f, n)).astype(np.int64)
    if kind == "low_luma":
        y = rng.integers(0, yoff + 1, (f, h, w))
    elif kind == "chroma_ends":
        c = np.where(rng.integers(0, 2, (2, f, ch, cw)) == 0, 0, P)
    elif kind not in ("legal", "low_bits"):
        raise ValueError(kind)
    words = join(y, c[0], c[1], fmt, lay)
    if kind == "low_bits":
        words = words | rng.integers(0, 1 << sh, words.shape)
    return words


def input_classes(fmt, lay):
    return YF.INPUT_CLASSES + (["low_bits"] if msb_shift(fmt, lay) else [])


# ---------------------------------------------------------------------------
# output: float RGB -> words

def levels_to_planes(q, fmt, lay):
    """int64 levels [F, 3, h, w] -> values Y, U, V."""
    t = table(fmt)
    P, yoff, coff = t[:3]
    yr, yg, yb, ur, ug, ub, vr, vg, vb = t[9:]
    f, _, h, w = q.shape
    by, bx = block(lay)
    sh = 20 + {1: 0, 2: 1, 4: 2}[by * bx]
    y = (yr * q[:, 0] + yg * q[:, 1] + yb * q[:, 2] + (yoff << 20) + (1 << 19)) >> 20
    s = q.reshape(f, 3, h // by, by, w // bx, bx).sum(axis=(3, 5))
    u = (ur * s[:, 0] + ug * s[:, 1] + ub * s[:, 2] + (coff << sh) + (1 << (sh - 1))) >> sh
    v = (vr * s[:, 0] + vg * s[:, 1] + vb * s[:, 2] + (coff << sh) + (1 << (sh - 1))) >> sh
    return tuple(np.clip(p, 0, P) for p in (y, u, v))


def rgb_to_yuv(rgb, fmt, lay):
    """[F, 3, H, W] float -> the frames' words, int64 [F, n]."""
    q = YF.quantize(np.asarray(rgb, F32), table(fmt)[0])
    return join(*levels_to_planes(q, fmt, lay), fmt, lay)


def sse(words, ref_words, h, w, fmt, lay):
    """Exact sums of squared differences of the VALUES, int64 [F, 3] (Y, U, V)."""
    a, b = split(words, h, w, fmt, lay), split(ref_words, h, w, fmt, lay)
    return np.stack([((p - r) ** 2).reshape(p.shape[0], -1).sum(1) for p, r in zip(a, b)], axis=1)


def psnr_counts(lay, h, w):
    ch, cw = chroma_shape(lay, h, w)
    return h * w, ch * cw, ch * cw


def values(kind, f, h, w, P, seed=0):
    return YF.values(kind, f, h, w, P, seed)


def reference_words(f, h, w, fmt, lay, seed=0):
    """Random source frames over the whole sample word (low bits of the P010
    family included)."""
    rng = np.random.default_rng(seed * 77 + h * 3 + w + fmt[0] + layout_code(lay))
    return rng.integers(0, 256 if fmt[0] == 8 else 65536, (f, frame_samples(lay, h, w))).astype(np.int64)


def planar420_values(rgb, fmt):
    """What the existing planar 4:2:0 kernels write for ``rgb``, as values
    [F, h*w*3/2]: yuv_cases for the legacy triple, yuv_format_cases otherwise."""
    if tuple(fmt) == YF.LEGACY:
        return Y.rgb_to_i420(rgb).astype(np.int64)
    return YF.rgb_to_yuv420(rgb, fmt)
