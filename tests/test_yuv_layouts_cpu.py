"""CPU: 4:2:2, 4:4:4 and semi-planar YUV (csrc/yuv_conv.hip, the ``chroma`` and
``layout`` of ``video.YuvFormat``): the descriptor and ffmpeg's names, the
premises of the arithmetic per layout, known answers in every layout, the
byte permutation nv12 is of I420, the 4:4:4 round trip, the torch dispatch of
both conversions against the numpy statement (tests/yuv_layout_cases.py), the
C entries' argument errors, the container's layout word, the CPU
``decode_video`` and the command lines."""
import ctypes
import json
import struct

import numpy as np
import pytest
import torch

import yuv_cases as Y
import yuv_format_cases as YF
import yuv_layout_cases as YL

from gsvc_amd import codec
from gsvc_amd import compress as C
from gsvc_amd import video
from gsvc_amd.video import YuvFormat, i420_to_rgb, rgb_to_i420

H, W = 32, 48
GOP = [(65, True), (50, False), (33, False), (71, True), (41, False)]  # (splats, key frame)
TEN = (10, "bt709", False)

lay_param = pytest.mark.parametrize("lay", YL.NEW_LAYOUTS, ids=YL.lay_id)
all_lay_param = pytest.mark.parametrize("lay", YL.ALL_LAYOUTS, ids=YL.lay_id)


def _fmt(f, lay=YL.PLANAR420):
    return YuvFormat(f[0], f[1], f[2], lay[0], lay[1])


# --------------------------------------------------------------------------
# the descriptor and the names

def test_descriptor_defaults_and_sizes():
    d = YuvFormat()
    assert (d.chroma, d.layout, d.layout_code) == ("420", "planar", 0) and d.is_legacy
    assert YuvFormat(10, "bt709", False) == YuvFormat(10, "bt709", False, "420", "planar")  # positional, as before
    assert str(YuvFormat(10, "bt709")) == "10-bit bt709 limited range"  # a default-layout format prints as before
    assert "4:2:2" in str(YuvFormat(10, "bt709", chroma="422")) and "semi" in str(YuvFormat(layout="semi"))
    seen = set()
    for f in YF.ALL_FORMATS:
        for lay in YL.ALL_LAYOUTS:
            d = _fmt(f, lay)
            seen.add(d)
            assert d.is_legacy == (f == YF.LEGACY and lay == YL.PLANAR420)
            assert d.flags == YF.flags(f)  # the colour triple only
            assert d.layout_code == YL.layout_code(lay)
            assert YuvFormat.from_flags(d.flags, d.layout_code) == d
            assert d.frame_bytes(H, W) == YL.frame_bytes(f, lay, H, W)
            assert tuple(d.plane_shapes(H, W)) == YL.plane_shapes(lay, H, W)
            assert list(d.table()) == YF.table(f)  # the query keeps returning what it returns
    assert len(seen) == 16 * 6
    assert YuvFormat(chroma="444").frame_bytes(3, 5) == 45 and YuvFormat(10, chroma="422").frame_bytes(3, 6) == 72
    assert tuple(YuvFormat(chroma="444", layout="semi").plane_shapes(3, 5)) == ((3, 5), (3, 10))
    for bad in ((3, 6, "420"), (4, 5, "420"), (3, 5, "422"), (0, 4, "444"), (4, -2, "444")):
        with pytest.raises(ValueError):
            YuvFormat(chroma=bad[2]).plane_shapes(bad[0], bad[1])
    for chroma in ("411", "440", "", None, 4):
        with pytest.raises(ValueError, match="chroma"):
            YuvFormat(chroma=chroma)
    for layout in ("packed", "nv21", "", None):
        with pytest.raises(ValueError, match="layout"):
            YuvFormat(layout=layout)
    with pytest.raises(Exception):
        d.chroma = "444"  # frozen


def test_layout_codes():
    """Bits 0-1 chroma (0, 1, 2), bit 4 semi-planar; everything else is refused."""
    assert YuvFormat(chroma="422").layout_code == 1 and YuvFormat(chroma="444", layout="semi").layout_code == 0x12
    good = {0, 1, 2, 0x10, 0x11, 0x12}
    for code in list(range(64)) + [1 << b for b in range(6, 32)] + [0x10 | 1 << b for b in range(6, 32)]:
        if code in good:
            assert YuvFormat.from_flags(0x11, code).layout_code == code
        else:
            with pytest.raises(ValueError, match="unknown layout code"):
                YuvFormat.from_flags(0x11, code)
    with pytest.raises(ValueError, match="unknown file flags"):  # the flags still code the triple only
        YuvFormat.from_flags(0x04, 1)


def test_pix_fmt_names_both_ways():
    """Every depth x chroma x layout has ffmpeg's name, and the name gives it back."""
    assert len(YL.PIX_FMTS) == 24 == len(set(YL.PIX_FMTS.values()))
    for (b, c, l), name in YL.PIX_FMTS.items():
        d = YuvFormat(b, "bt709", True, c, l)
        assert d.pix_fmt == name
        assert YuvFormat.from_pix_fmt(name) == YuvFormat(b, "bt601", False, c, l)  # matrix, range: not in a name
        assert YuvFormat.from_pix_fmt(name, "bt709", True) == d
    assert YuvFormat().pix_fmt == "yuv420p" and YuvFormat.from_pix_fmt("yuv420p").is_legacy
    for name in ("yuv420p10", "nv21", "p010", "yuv411p", "yuyv422", "", "P010LE"):
        with pytest.raises(ValueError, match="pix_fmt"):
            YuvFormat.from_pix_fmt(name)


# --------------------------------------------------------------------------
# premises and known answers

@pytest.mark.parametrize("fmt", YF.ALL_FORMATS, ids=YF.fmt_id)
def test_premises_per_layout(fmt):
    """With the table each layout computes with (the legacy kernels' constants
    for the legacy triple): the accumulators stay below 2^39 at the extreme
    inputs, and at 8 bits below 2^31 in magnitude, where the kernels keep them
    in int32; the chroma accumulator of a block of n pixels is no larger than
    the 2x2 block's, so yuv_format_cases' bound covers it."""
    t = YL.table(fmt)
    P, yoff, coff = t[:3]
    top = 255 if fmt[0] == 8 else 65535  # any sample word (a P010 word's value is at most P)
    cy, crv, cgu, cgv, cbu = t[4:9]
    worst_in = (top * cy + (1 << 19)) + top * max(abs(crv), abs(cgu) + abs(cgv), abs(cbu))
    worst_y = (yoff << 20) + (1 << 19) + P * sum(abs(c) for c in t[9:12])
    per_n = {}
    for n, sh in ((4, 22), (2, 21), (1, 20)):
        per_n[n] = max((coff << sh) + (1 << (sh - 1)) + n * P * sum(abs(c) for c in coef) for coef in (t[12:15], t[15:18]))
    assert per_n[1] < per_n[2] < per_n[4]
    worst = max(worst_in, worst_y, per_n[4])
    assert worst < 2 ** 39
    if fmt[0] == 8:
        assert worst < 2 ** 31
    else:
        assert worst > 2 ** 31  # int64 is needed from 10 bits up, at 4:4:4 too:
        assert max(worst_in, worst_y) > 2 ** 31


def _flat(rgb, fmt, lay, h=2, w=2):
    img = np.broadcast_to(np.array(rgb, np.float32).reshape(1, 3, 1, 1), (1, 3, h, w))
    y, u, v = YL.split(YL.rgb_to_yuv(img, fmt, lay), h, w, fmt, lay)
    assert len(set(y.reshape(-1).tolist())) == len(set(u.reshape(-1).tolist())) == len(set(v.reshape(-1).tolist())) == 1
    return int(y[0, 0, 0]), int(u[0, 0, 0]), int(v[0, 0, 0])


@all_lay_param
@pytest.mark.parametrize("fmt, rgb, yuv", [
    (TEN, (0, 0, 0), (64, 512, 512)), (TEN, (1, 1, 1), (940, 512, 512)), (TEN, (1, 0, 0), (250, 409, 960)),
    ((10, "bt601", False), (1, 0, 0), (326, 361, 960)), ((8, "bt709", False), (1, 0, 0), (63, 102, 240))])
def test_known_answers_in_every_layout(fmt, rgb, yuv, lay):
    """DESIGN.md §13e's answers: a flat frame's values do not depend on the layout."""
    assert _flat(rgb, fmt, lay) == yuv
    if lay == YL.PLANAR420:
        return
    img = torch.tensor(rgb, dtype=torch.float32).view(1, 3, 1, 1).expand(1, 3, 2, 2)
    words = YL.from_bytes(rgb_to_i420(img, fmt=_fmt(fmt, lay)).numpy(), fmt)
    got = [int(p[0, 0, 0]) for p in YL.split(words, 2, 2, fmt, lay)]
    assert tuple(got) == yuv
    sh = YL.msb_shift(fmt, lay)
    assert set(words[0].tolist()) == {v << sh for v in yuv}


def test_ten_bit_red_in_the_msb_form():
    """p010le / p210le / p410le of 10-bit BT.709 limited red: (16000, 26176, 61440)."""
    img = torch.tensor((1.0, 0.0, 0.0)).view(1, 3, 1, 1).expand(1, 3, 2, 2)
    for name, count in (("p010le", (4, 1)), ("p210le", (4, 2)), ("p410le", (4, 4))):
        d = YuvFormat.from_pix_fmt(name, "bt709")
        words = YL.from_bytes(rgb_to_i420(img, fmt=d).numpy(), TEN)[0].tolist()
        ny, nc = count
        assert words == [16000] * ny + [26176, 61440] * nc, name
        assert (250 << 6, 409 << 6, 960 << 6) == (16000, 26176, 61440)
        # and back: the low bits of a word are ignored
        noisy = torch.from_numpy((np.array(words) | 0x3f).astype(np.uint16).view(np.uint8).copy())
        clean = torch.from_numpy(np.array(words).astype(np.uint16).view(np.uint8).copy())
        assert torch.equal(i420_to_rgb(noisy, 2, 2, d), i420_to_rgb(clean, 2, 2, d))


@pytest.mark.parametrize("fmt", YF.ALL_FORMATS, ids=YF.fmt_id)
def test_flat_frames_do_not_depend_on_the_layout(fmt):
    """(4a) >> 22 = (2a) >> 21 = a >> 20: flat blocks give the same sample values in all six layouts."""
    rng = np.random.default_rng(fmt[0])
    for rgb in rng.uniform(0, 1, (12, 3)).tolist() + [(0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)]:
        got = {lay: _flat(rgb, fmt, lay) for lay in YL.NEW_LAYOUTS}
        if fmt == YF.LEGACY:  # planar 4:2:0: the legacy kernel's statement
            img = np.broadcast_to(np.array(rgb, np.float32).reshape(1, 3, 1, 1), (1, 3, 2, 2))
            want = tuple(int(v) for v in Y.rgb_to_i420(img)[0, 3:])
        else:
            want = _flat(rgb, fmt, YL.PLANAR420)
        assert all(v == want for v in got.values()), (rgb, got, want)


# --------------------------------------------------------------------------
# nv12 / p010 are a permutation of planar 4:2:0

@pytest.mark.parametrize("fmt", YF.ALL_FORMATS, ids=YF.fmt_id)
def test_semi_planar_420_is_a_permutation_of_planar_420(fmt):
    lay = ("420", "semi")
    d, P = _fmt(fmt, lay), YF.spans(fmt)[0]
    for h, w in ((2, 2), (6, 10), (18, 24)):
        x = YF.values("uniform", 2, h, w, P) if fmt != YF.LEGACY else Y.values("uniform", 2, h, w)
        planar = YL.planar420_values(x, fmt)  # what today's kernels write
        want = YL.i420_to_layout(planar, h, w, fmt, lay)
        assert np.array_equal(YL.rgb_to_yuv(x, fmt, lay), want)
        got = rgb_to_i420(torch.from_numpy(x), fmt=d).numpy()
        assert np.array_equal(got, YL.to_bytes(want, fmt))
        if fmt[0] == 8:  # the same bytes, in another order
            assert sorted(got[0].tolist()) == sorted(YL.to_bytes(planar, fmt)[0].tolist())
        # input: the floats today's conversion gives for the de-interleaved planes
        s = YF.input_values("legal", 1, h, w, fmt)
        semi = YL.i420_to_layout(s, h, w, fmt, lay)
        today = i420_to_rgb(torch.from_numpy(YF.to_bytes(s, fmt)[0].copy()), h, w, _fmt(fmt))
        assert torch.equal(i420_to_rgb(torch.from_numpy(YL.to_bytes(semi, fmt)[0].copy()), h, w, d), today)
        assert np.array_equal(YL.yuv_to_rgb(semi, h, w, fmt, lay), today.numpy())


# --------------------------------------------------------------------------
# the 4:4:4 round trip

@pytest.mark.parametrize("fmt", YF.ALL_FORMATS, ids=YF.fmt_id)
def test_round_trip_444(fmt):
    """200 000 seeded pixels, uniform over the legal codes, as one 4:4:4 row:
    where the inverse does not clip (at least 20 % of them; this draw gives
    23.5-24.5 %, as the flat 2x2 blocks of DESIGN.md §13e), forward o inverse
    returns U and V exactly and Y within 1 (exactly in 14 of the 16 triples;
    one level off at the legacy triple's three-decimal constants and at 16-bit
    bt709 full).  4:4:4 keeps every source sample, so this is the loop's loss."""
    lay = ("444", "planar")
    P, yoff, coff, ys, cs = YF.spans(fmt)
    rng = np.random.default_rng(1)
    n = 200000
    clo, chi = (0, P) if fmt[2] else (coff - cs // 2, coff + cs // 2)
    y, u, v = (rng.integers(yoff, yoff + ys + 1, n), rng.integers(clo, chi + 1, n), rng.integers(clo, chi + 1, n))
    words = YL.join(y.reshape(1, 1, n), u.reshape(1, 1, n), v.reshape(1, 1, n), fmt, lay)
    raw = YL.yuv_to_rgb_int(words, 1, n, fmt, lay, clamp=False)[0]
    ok = ((raw >= 0) & (raw <= P)).all(axis=(0, 1))
    share = ok.mean()
    back = YL.split(YL.rgb_to_yuv(YL.yuv_to_rgb(words, 1, n, fmt, lay), fmt, lay), 1, n, fmt, lay)
    worst = [int(np.abs(a.reshape(-1) - b)[ok].max()) for a, b in zip(back, (y, u, v))]
    print(f"{YF.fmt_id(fmt)} 4:4:4: unclipped share {share:.4f}, max errors {worst}")
    assert 0.20 <= share and 0.235 <= round(share, 3) <= 0.246
    assert worst[0] <= 1 and worst[1:] == [0, 0]


# --------------------------------------------------------------------------
# the torch dispatch against the numpy statement

@lay_param
@pytest.mark.parametrize("fmt", YL.GPU_FORMATS + [(8, "bt709", True)], ids=YF.fmt_id)
def test_torch_output_equals_numpy(fmt, lay):
    d, P = _fmt(fmt, lay), YF.spans(fmt)[0]
    for h, w in YL.SHAPES:
        if not YL.fits(lay, h, w):
            with pytest.raises(ValueError):
                rgb_to_i420(torch.zeros(1, 3, h, w), fmt=d)
            continue
        for f in YL.FRAMES:
            for kind in YF.CLASSES:
                x = YL.values(kind, f, h, w, P)
                want = YL.rgb_to_yuv(x, fmt, lay)
                got = rgb_to_i420(torch.from_numpy(x), fmt=d)
                assert got.dtype == torch.uint8 and got.shape == (f, d.frame_bytes(h, w))
                assert np.array_equal(got.numpy(), YL.to_bytes(want, fmt)), (h, w, f, kind)
            ref = YL.reference_words(f, h, w, fmt, lay)
            got2, sse = rgb_to_i420(torch.from_numpy(x), torch.from_numpy(YL.to_bytes(ref, fmt)), fmt=d)
            assert np.array_equal(got2.numpy(), YL.to_bytes(want, fmt))
            assert sse.dtype == torch.int64 and np.array_equal(sse.numpy(), YL.sse(want, ref, h, w, fmt, lay))
            _, zero = rgb_to_i420(torch.from_numpy(x), got2, fmt=d)
            assert not zero.any()


@lay_param
@pytest.mark.parametrize("fmt", YL.GPU_FORMATS + [(8, "bt709", True)], ids=YF.fmt_id)
def test_torch_input_equals_numpy(fmt, lay):
    d = _fmt(fmt, lay)
    for h, w in YL.SHAPES:
        if not YL.fits(lay, h, w):
            with pytest.raises(ValueError):
                i420_to_rgb(torch.zeros(d.frame_bytes(h, w), dtype=torch.uint8), h, w, d)
            continue
        for kind in YL.input_classes(fmt, lay):
            s = YL.input_values(kind, 1, h, w, fmt, lay)
            want = YL.yuv_to_rgb(s, h, w, fmt, lay)
            got = i420_to_rgb(torch.from_numpy(YL.to_bytes(s, fmt)[0].copy()), h, w, d)
            assert got.dtype == torch.float32 and got.shape == (1, 3, h, w)
            assert np.array_equal(got.numpy(), want), (h, w, kind)
            if d.sample_bytes == 2:  # the samples themselves, as int16
                words = torch.from_numpy(s[0].astype(np.uint16).view(np.int16).copy())
                assert np.array_equal(i420_to_rgb(words, h, w, d).numpy(), want)
    with pytest.raises(ValueError):
        i420_to_rgb(torch.zeros(5, dtype=torch.uint8), 2, 2, d)


def test_planar_420_still_takes_the_calls_of_before():
    """No layout named: the conversions of before, byte for byte."""
    x = Y.values("uniform", 2, 6, 10)
    assert np.array_equal(rgb_to_i420(torch.from_numpy(x), fmt=YuvFormat(8, "bt601", False, "420", "planar")).numpy(),
                          Y.rgb_to_i420(x))
    x10 = YF.values("uniform", 2, 6, 10, 1023)
    assert np.array_equal(rgb_to_i420(torch.from_numpy(x10), fmt=YuvFormat(*TEN, "420", "planar")).numpy(),
                          YF.to_bytes(YF.rgb_to_yuv420(x10, TEN), TEN))


# --------------------------------------------------------------------------
# the C entries' argument checks

def test_c_entries_argument_errors_without_launch():
    from gsvc_amd import _lib
    lib = _lib.load()
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(65)  # never dereferenced: the argument checks fail first

    def f(*v):
        return (ctypes.c_int * 3)(*v)

    ten, legacy, eight = f(10, 1, 0), f(8, 0, 0), f(8, 1, 0)
    # (frames, rgb, h, w, fmt, chroma, semi, out, ref, sse)
    out_cases = [((1, p, 2, 2, ten, 420, 0, p, None, None), b"planar 4:2:0"),
                 ((1, p, 2, 2, legacy, 420, 0, p, None, None), b"planar 4:2:0"),
                 ((1, p, 2, 2, ten, 421, 1, p, None, None), b"chroma"), ((1, p, 2, 2, ten, 0, 1, p, None, None), b"chroma"),
                 ((1, p, 2, 2, ten, 2, 1, p, None, None), b"chroma"), ((1, p, 2, 2, ten, 422, 2, p, None, None), b"semi_planar"),
                 ((1, p, 2, 2, f(9, 1, 0), 422, 0, p, None, None), b"bit_depth"),
                 ((1, p, 2, 2, f(10, 2, 0), 422, 0, p, None, None), b"matrix"),
                 ((1, p, 2, 2, f(10, 1, 2), 444, 1, p, None, None), b"full_range"),
                 ((1, p, 2, 2, None, 444, 0, p, None, None), b"missing format"),
                 ((0, p, 2, 2, ten, 422, 0, p, None, None), b"frames"), ((-3, p, 2, 2, ten, 444, 1, p, None, None), b"frames"),
                 ((1, p, 3, 2, ten, 420, 1, p, None, None), b"even"), ((1, p, 2, 3, ten, 420, 1, p, None, None), b"even"),
                 ((1, p, 3, 3, ten, 422, 0, p, None, None), b"even width"), ((1, p, 2, 7, ten, 422, 1, p, None, None), b"even width"),
                 ((1, p, 0, 2, ten, 444, 0, p, None, None), b"positive"), ((1, p, 3, -5, ten, 444, 1, p, None, None), b"positive"),
                 ((1, None, 2, 2, ten, 444, 0, p, None, None), b"missing buffer"),
                 ((1, p, 2, 2, ten, 444, 0, None, None, None), b"missing buffer"),
                 ((1, p, 2, 2, ten, 422, 1, p, p, None), b"sse"), ((1, p, 2, 2, eight, 420, 1, p, p, None), b"sse"),
                 ((1, p, 2, 2, ten, 422, 0, odd, None, None), b"odd address"),
                 ((1, p, 2, 2, ten, 444, 1, p, odd, p), b"odd address")]
    for args, msg in out_cases:
        assert lib.gsvc_rgb_to_yuv(*args, None) == 1, args
        assert msg in lib.gsvc_last_error(), (args, lib.gsvc_last_error())
    # (frames, yuv, h, w, fmt, chroma, semi, out)
    in_cases = [((1, p, 2, 2, ten, 420, 0, p), b"planar 4:2:0"), ((1, p, 2, 2, legacy, 420, 0, p), b"planar 4:2:0"),
                ((1, p, 2, 2, ten, 411, 0, p), b"chroma"), ((1, p, 2, 2, f(9, 1, 0), 444, 0, p), b"bit_depth"),
                ((-1, p, 2, 2, ten, 422, 0, p), b"frames"), ((1, p, 2, 5, ten, 422, 0, p), b"even width"),
                ((1, p, 5, 2, ten, 420, 1, p), b"even"), ((1, p, -2, 2, ten, 444, 0, p), b"positive"),
                ((1, None, 2, 2, ten, 444, 0, p), b"missing buffer"), ((1, p, 2, 2, ten, 444, 0, None), b"missing buffer"),
                ((1, odd, 2, 2, ten, 422, 1, p), b"odd address")]
    for args, msg in in_cases:
        assert lib.gsvc_yuv_to_rgb(*args, None) == 1, args
        assert msg in lib.gsvc_last_error(), (args, lib.gsvc_last_error())
    assert lib.gsvc_abi_version() == 4


# --------------------------------------------------------------------------
# the container

def _gop_cpu(plan=GOP, h=H, w=W, seed=5):
    """As tests/test_yuv_formats_cpu.py: frame streams of untrained models on the
    CPU, every delta on the decoded parameters of the frame before it."""
    torch.manual_seed(seed)
    kw = dict(H=h, W=w, BLOCK_H=16, BLOCK_W=16, device="cpu", lr=1e-3, quantize=True, opt_type="adan")
    streams, state = [], None
    for k, (n, key) in enumerate(plan):
        if key:
            m = C.GaussianVideoFrameQ(num_points=n, **kw)
            with torch.no_grad():
                m._cholesky.mul_(3.0)
            state = None
        else:
            m = C.GaussianVideoDelta(num_points=n, **kw)
            with torch.no_grad():
                m._xyz.copy_(0.05 * torch.randn(n, 2))
                m._cholesky.copy_(0.3 * torch.randn(n, 3))
                m._features_dc.copy_(0.1 * torch.randn(n, 3))
                m.p_xyz.copy_(torch.from_numpy(state[0][:n]))
                m.p_cholesky.copy_(torch.from_numpy(state[1][:n]))
                m.p_features_dc.copy_(torch.from_numpy(state[2][:n]))
        m._init_data()
        m.eval()
        s = C.encode_frame(m, entropy=bool(k & 1), segment=16)
        xq, _, cq, Lpre = C.unpack_frames_host([s], prev=state)[0]
        state = (xq, Lpre, cq)
        streams.append(s)
    return streams


@pytest.fixture(scope="module")
def gop():
    streams = _gop_cpu()
    return streams, C.decode_frames(streams, "cpu").numpy()


def _file_of_before(streams, flags, fps=(30, 1)):
    """The container as DESIGN.md §13d / §13e lay it out, written here by hand:
    48 header bytes, 16 zero bytes, the streams, the index."""
    heads = [C.parse_header(s) for s in streams]
    off, index = 64, []
    for s, h in zip(streams, heads):
        index.append(struct.pack("<QII", off, len(s), 1 if h["delta"] else 0))
        off += len(s)
    head = struct.pack("<4sIIIIIIIQQ", b"GSVF", 1, heads[0]["H"], heads[0]["W"], len(streams), fps[0], fps[1], flags,
                       off, off + 16 * len(streams))
    return head + bytes(16) + b"".join(streams) + b"".join(index)


def test_header_layout_word(gop, tmp_path):
    streams, _ = gop
    path = tmp_path / "a.gsvf"
    for f in YF.ALL_FORMATS:  # the 16 default-layout formats: the bytes of before
        codec.write_video(path, streams, fmt=_fmt(f))
        assert path.read_bytes() == _file_of_before(streams, YF.flags(f))
    codec.write_video(path, streams)
    plain = path.read_bytes()
    assert plain == _file_of_before(streams, 0) and codec.read_video(path).format == YuvFormat()
    for lay in YL.ALL_LAYOUTS:
        for f in (YF.LEGACY, TEN, (16, "bt601", True)):
            codec.write_video(path, streams, fmt=_fmt(f, lay))
            blob = path.read_bytes()
            assert struct.unpack_from("<II", blob, 4) == (1, H)  # still version 1
            assert struct.unpack_from("<I", blob, 28)[0] == YF.flags(f)
            assert struct.unpack_from("<I", blob, 48)[0] == YL.layout_code(lay)
            assert blob[:28] == plain[:28] and blob[32:48] == plain[32:48] and blob[52:] == plain[52:]
            vid = codec.read_video(path)
            assert vid.format == _fmt(f, lay) and vid.num_frames == len(streams)
    for code in (3, 4, 8, 0x13, 0x20, 0x100, 1 << 31):
        bad = bytearray(plain)
        struct.pack_into("<I", bad, 48, code)
        path.write_bytes(bytes(bad))
        with pytest.raises(ValueError, match="unknown layout code"):
            codec.read_video(path)
        with pytest.raises(ValueError, match="unknown layout code"):
            codec.decode_video(str(path), device="cpu")
    for at in range(52, 64):
        bad = bytearray(plain)
        bad[at] = 1
        struct.pack_into("<I", bad, 48, 0x11)
        path.write_bytes(bytes(bad))
        with pytest.raises(ValueError, match="reserved header bytes"):
            codec.read_video(path)


def test_decode_frames_cpu_layouts(gop):
    streams, imgs = gop
    for name in ("nv12", "yuv422p10le", "yuv444p", "p010le"):
        d = YuvFormat.from_pix_fmt(name, "bt709")
        f, lay = (d.bit_depth, "bt709", False), (d.chroma, d.layout)
        want = YL.to_bytes(YL.rgb_to_yuv(imgs[:3], f, lay), f)
        for output in ("yuv", "i420"):
            out = C.decode_frames(streams[:3], "cpu", output=output, fmt=d)
            assert out.shape == (3, d.frame_bytes(H, W)) and np.array_equal(out.numpy(), want), (name, output)
    assert np.array_equal(C.decode_frames(streams[:3], "cpu", output="yuv", fmt=YuvFormat()).numpy(),
                          Y.rgb_to_i420(imgs[:3]))
    with pytest.raises(ValueError):  # "yuv" names a format's frames: without one it stays an error
        C.decode_frames(streams[:3], "cpu", output="yuv")
    with pytest.raises(ValueError):
        C.decode_frames(streams[:3], "cpu", output="nv12")
    with pytest.raises(ValueError):
        C.decode_frames(streams[:3], "cpu", fmt=YuvFormat(layout="semi"))  # a format without output="yuv"


@pytest.mark.parametrize("name, fmt", [("nv12", YF.LEGACY), ("yuv444p10le", TEN)])
def test_decode_video_cpu_layouts(gop, tmp_path, name, fmt):
    streams, imgs = gop
    d = YuvFormat.from_pix_fmt(name, fmt[1], fmt[2])
    lay = (d.chroma, d.layout)
    size = d.frame_bytes(H, W)
    want = YL.rgb_to_yuv(imgs, fmt, lay)
    path = tmp_path / "v.gsvf"
    codec.write_video(path, streams, fmt=d)
    src = YL.input_values("legal", 5, H, W, fmt, lay, seed=3)
    (tmp_path / "src.yuv").write_bytes(YL.to_bytes(src, fmt).tobytes())
    res = codec.decode_video(str(path), str(tmp_path / "out.yuv"), device="cpu", batch=2,
                             reference=str(tmp_path / "src.yuv"))
    assert res["frames"] == 5 and res["bytes_written"] == 5 * size
    assert (tmp_path / "out.yuv").read_bytes() == YL.to_bytes(want, fmt).tobytes()
    e = YL.sse(want, src, H, W, fmt, lay)
    counts = YL.psnr_counts(lay, H, W)
    assert counts == ((H * W, H * W // 4, H * W // 4) if name == "nv12" else (H * W,) * 3)
    for f in range(5):
        p = [YF.psnr(e[f, k], counts[k], d.peak) for k in range(3)]
        assert (res["psnr_y"][f], res["psnr_u"][f], res["psnr_v"][f]) == pytest.approx(p, rel=1e-12)
        assert res["psnr_yuv"][f] == pytest.approx((6 * p[0] + p[1] + p[2]) / 8, rel=1e-12)
    (tmp_path / "same.yuv").write_bytes(YL.to_bytes(want, fmt).tobytes())
    same = codec.decode_video(str(path), device="cpu", reference=str(tmp_path / "same.yuv"))
    assert all(np.isinf(p) for k in ("psnr_y", "psnr_u", "psnr_v", "psnr_yuv") for p in same[k])
    part = codec.decode_video(str(path), str(tmp_path / "part.yuv"), device="cpu", batch=2, frames=range(3, 5))
    assert part["bytes_written"] == 2 * size
    assert (tmp_path / "part.yuv").read_bytes() == YL.to_bytes(want[3:5], fmt).tobytes()
    # fmt= re-targets: the file back to planar 4:2:0 of the same triple is today's output
    codec.decode_video(str(path), str(tmp_path / "p.yuv"), device="cpu", fmt=_fmt(fmt))
    assert (tmp_path / "p.yuv").read_bytes() == YF.to_bytes(YL.planar420_values(imgs, fmt), fmt).tobytes()


def test_decode_video_refuses_an_odd_width_at_422(tmp_path):
    streams = _gop_cpu([(20, True)], h=6, w=7)
    with pytest.raises(ValueError, match="even width"):
        codec.decode_video(streams, device="cpu", fmt=YuvFormat(chroma="422"))
    res = codec.decode_video(streams, str(tmp_path / "o.yuv"), device="cpu", fmt=YuvFormat(chroma="444", layout="semi"))
    assert res["bytes_written"] == 3 * 6 * 7  # 4:4:4 takes any size


# --------------------------------------------------------------------------
# the command lines

def _source(tmp_path, fmt, lay, h=32, w=48, frames=3):
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    ch, cw = YL.chroma_shape(lay, h, w)
    ys, us, vs = [], [], []
    for f in range(frames):
        ys.append((xx * 17 + yy * 11 + 80 * f) % 876 + 64)
        us.append(np.full((ch, cw), 400 + 40 * f))
        vs.append(np.full((ch, cw), 560))
    src = YL.join(np.stack(ys), np.stack(us), np.stack(vs), fmt, lay)
    (tmp_path / "src.yuv").write_bytes(YL.to_bytes(src, fmt).tobytes())
    return src


def test_cli_encode_info_decode_p010(tmp_path, capsys):
    h, w, frames, n = 32, 48, 3, 40
    lay = ("420", "semi")
    _source(tmp_path, TEN, lay, h, w, frames)
    g = torch.Generator().manual_seed(11)
    models = {f"frame_{f + 1}": {"_xyz": torch.atanh(1.8 * (torch.rand(n, 2, generator=g) - 0.5)),
                                 "_cholesky": 3.0 * torch.rand(n, 3, generator=g),
                                 "_features_dc": torch.rand(n, 3, generator=g)} for f in range(frames)}
    torch.save(models, tmp_path / "models.pth")
    enc = codec.main(["encode", str(tmp_path / "models.pth"), str(tmp_path / "src.yuv"), str(tmp_path / "v.gsvf"),
                      "--width", str(w), "--height", str(h), "--iterations", "2", "--k_frames", "1,3",
                      "--seed", "3", "--device", "cpu", "--pix_fmt", "p010le", "--matrix", "bt709"])
    assert enc["frames"] == frames
    d = _fmt(TEN, lay)
    assert codec.read_video(tmp_path / "v.gsvf").format == d
    capsys.readouterr()
    info = codec.main(["info", str(tmp_path / "v.gsvf")])
    assert json.loads(capsys.readouterr().out) == info
    assert info["format"] == {"bit_depth": 10, "matrix": "bt709", "full_range": False}
    assert (info["chroma"], info["layout"], info["pix_fmt"]) == ("420", "semi", "p010le")
    size = d.frame_bytes(h, w)
    dec = codec.main(["decode", str(tmp_path / "v.gsvf"), str(tmp_path / "out.yuv"), "--device", "cpu",
                      "--batch", "2", "--reference", str(tmp_path / "src.yuv")])
    assert (tmp_path / "out.yuv").stat().st_size == frames * size == dec["bytes_written"]
    assert len(dec["psnr_yuv"]) == frames and all(np.isfinite(dec["psnr_yuv"]))
    imgs = C.decode_frames([codec.read_video(tmp_path / "v.gsvf").frame(i) for i in range(frames)], "cpu").numpy()
    assert (tmp_path / "out.yuv").read_bytes() == YL.to_bytes(YL.rgb_to_yuv(imgs, TEN, lay), TEN).tobytes()
    # the override: one option leaves the file's others
    over = codec.main(["decode", str(tmp_path / "v.gsvf"), str(tmp_path / "o.yuv"), "--device", "cpu",
                       "--chroma", "444", "--layout", "planar"])
    l2 = ("444", "planar")
    assert over["bytes_written"] == frames * h * w * 3 * 2
    assert (tmp_path / "o.yuv").read_bytes() == YL.to_bytes(YL.rgb_to_yuv(imgs, TEN, l2), TEN).tobytes()
    over = codec.main(["decode", str(tmp_path / "v.gsvf"), str(tmp_path / "o8.yuv"), "--device", "cpu",
                       "--pix_fmt", "nv16"])
    f8, l3 = (8, "bt709", False), ("422", "semi")
    assert (tmp_path / "o8.yuv").read_bytes() == YL.to_bytes(YL.rgb_to_yuv(imgs, f8, l3), f8).tobytes()
    # --pix_fmt beside a different --bit_depth / --chroma / --layout is an error; the same value is not
    for extra in (["--bit_depth", "8"], ["--chroma", "422"], ["--layout", "planar"]):
        with pytest.raises(ValueError, match="pix_fmt"):
            codec.main(["decode", str(tmp_path / "v.gsvf"), str(tmp_path / "x.yuv"), "--device", "cpu",
                        "--pix_fmt", "p010le"] + extra)
    same = codec.main(["decode", str(tmp_path / "v.gsvf"), str(tmp_path / "x.yuv"), "--device", "cpu",
                       "--pix_fmt", "p010le", "--bit_depth", "10", "--chroma", "420", "--layout", "semi"])
    assert same["bytes_written"] == frames * size


def test_video_cli_loads_a_422_ten_bit_dataset(tmp_path):
    """python -m gsvc_amd.video --dataset --pix_fmt yuv422p10le: the frames it
    trains on are that layout's conversion (read as 4:2:0 the file would hold
    four frames of the wrong bytes)."""
    lay = ("422", "planar")
    src = _source(tmp_path, TEN, lay)
    args = video.parse_args(["-d", str(tmp_path / "src.yuv"), "--width", "48", "--height", "32",
                             "--pix_fmt", "yuv422p10le", "--matrix", "bt709"])
    fmt = video.format_of_arguments(args)
    assert fmt == _fmt(TEN, lay) and video.format_of_arguments(video.parse_args([])) is None
    assert video.format_of_arguments(video.parse_args(["--chroma", "444"])) == YuvFormat(chroma="444")
    assert video.format_of_arguments(video.parse_args(["--layout", "semi", "--bit_depth", "12"])).pix_fmt == "p012le"
    with pytest.raises(ValueError, match="pix_fmt"):
        video.format_of_arguments(video.parse_args(["--pix_fmt", "nv12", "--chroma", "444"]))
    frames, total = video.load_yuv_frames(args.dataset, args.width, args.height, "cpu", fmt=fmt)
    assert total == 3 and sorted(frames) == [0, 1, 2]
    want = YL.yuv_to_rgb(src, 32, 48, TEN, lay)
    assert all(np.array_equal(frames[i].numpy()[0], want[i]) for i in range(3))
    assert video.load_yuv_frames(args.dataset, 48, 32, "cpu", fmt=_fmt(TEN))[1] == 4  # read as 4:2:0
