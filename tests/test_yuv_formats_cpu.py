"""CPU: the pixel formats beyond 8-bit BT.601 limited range (csrc/yuv_conv.hip,
``video.YuvFormat``): the coefficient table against its formula, the premises
of the arithmetic, known answers, the round trip, the torch dispatch of both
conversions against the numpy statement (tests/yuv_format_cases.py), the
legacy format's unchanged bytes, the C entries' argument errors, the
container's format flags, the CPU ``decode_video`` and the command lines."""
import ctypes
import json
import struct

import numpy as np
import pytest
import torch

import yuv_cases as Y
import yuv_format_cases as YF

from gsvc_amd import codec
from gsvc_amd import compress as C
from gsvc_amd import video
from gsvc_amd.video import YuvFormat, i420_to_rgb, rgb_to_i420

H, W = 32, 48
GOP = [(65, True), (50, False), (33, False), (71, True), (41, False)]  # (splats, key frame)
TEN = (10, "bt709", False)

fmt_param = pytest.mark.parametrize("fmt", YF.FORMATS, ids=YF.fmt_id)


def _fmt(f):
    return YuvFormat(*f)


# --------------------------------------------------------------------------
# the descriptor

def test_descriptor():
    legacy = YuvFormat()
    assert (legacy.bit_depth, legacy.matrix, legacy.full_range) == YF.LEGACY and legacy.is_legacy
    assert legacy.flags == 0 and YuvFormat.from_flags(0) == legacy
    assert len({_fmt(f) for f in YF.ALL_FORMATS} | {YuvFormat(10, "bt709")}) == 16  # hashable, by value
    with pytest.raises(Exception):
        legacy.bit_depth = 10  # frozen
    for f in YF.ALL_FORMATS:
        d = _fmt(f)
        assert d.peak == 2 ** f[0] - 1 and d.sample_bytes == (1 if f[0] == 8 else 2)
        assert d.frame_bytes(H, W) == H * W * 3 // 2 * d.sample_bytes == YF.frame_bytes(f, H, W)
        assert d.is_legacy == (f == YF.LEGACY)
        assert d.flags == YF.flags(f) and YuvFormat.from_flags(d.flags) == d
    for depth in (0, 7, 9, 11, 14, 32):
        with pytest.raises(ValueError):
            YuvFormat(depth)
    for matrix in ("bt2020", "BT709", "", None):
        with pytest.raises(ValueError):
            YuvFormat(8, matrix)


def test_flag_bits():
    """Bits 0-1 depth, 4 matrix, 6 range; every other bit is refused."""
    assert YuvFormat(10, "bt709", False).flags == 0x11 and YuvFormat(16, "bt601", True).flags == 0x43
    assert YuvFormat(12).flags == 2
    for bit in range(32):
        if bit in (0, 1, 4, 6):
            continue
        with pytest.raises(ValueError, match="unknown file flags"):
            YuvFormat.from_flags(1 << bit)
        with pytest.raises(ValueError, match="unknown file flags"):
            YuvFormat.from_flags(0x11 | 1 << bit)


# --------------------------------------------------------------------------
# the table and the premises

def _c_table(fmt):
    from gsvc_amd import _lib
    out = (ctypes.c_longlong * 18)()
    rc = _lib.load().gsvc_yuv_format_table((ctypes.c_int * 3)(fmt[0], YF.MATRICES.index(fmt[1]), int(fmt[2])), out)
    return rc, list(out)


@pytest.mark.parametrize("fmt", YF.ALL_FORMATS, ids=YF.fmt_id)
def test_table_equals_the_formula(fmt):
    rc, got = _c_table(fmt)
    assert rc == 0 and got == YF.table(fmt)
    assert list(_fmt(fmt).table()) == got


def test_table_of_ten_bit_bt709_limited():
    """DESIGN.md §13e's table."""
    t = YF.table(TEN)
    assert t == [1023, 64, 512, 2, 1224536, 1885354, -224265, -560439, 2221529,
                 190894, 642179, 64828, -105223, -353977, 459200, 459200, -417094, -42106]
    assert sum(t[12:15]) == 0 and sum(t[15:18]) == 0  # grey has neutral chroma
    assert abs(sum(t[9:12]) - 876 / 1023 * 2 ** 20) < 1.5  # white is Yoff + Yspan


@pytest.mark.parametrize("fmt", YF.ALL_FORMATS, ids=YF.fmt_id)
def test_premises(fmt):
    """No coefficient within 1e-6 of a rounding tie (none lies within 0.015 of
    one: the table does not depend on the evaluation order); the
    accumulators stay below 2^62 at the extreme inputs (below 2^39 in fact), and
    at 8 bits below 2^31 in magnitude, where the kernels keep them in int32."""
    for c in YF.real_coefficients(fmt):
        frac = c * 2.0 ** 20 - np.floor(c * 2.0 ** 20)
        assert abs(frac - 0.5) > 1e-6
    t = YF.table(fmt)
    P, yoff, coff = t[:3]
    top = 255 if fmt[0] == 8 else 65535  # any sample word
    cy, crv, cgu, cgv, cbu = t[4:9]
    worst = (top * cy + (1 << 19)) + top * max(abs(crv), abs(cgu) + abs(cgv), abs(cbu))
    for coef, bias, most in ((t[9:12], (yoff << 20) + (1 << 19), P), (t[12:15], (coff << 22) + (1 << 21), 4 * P),
                             (t[15:18], (coff << 22) + (1 << 21), 4 * P)):
        worst = max(worst, bias + most * sum(abs(c) for c in coef))
    assert worst < 2 ** 39 < 2 ** 62
    if fmt[0] == 8:
        assert worst < 2 ** 31
    else:
        assert worst > 2 ** 31  # int64 is needed from 10 bits up


def _flat(rgb, fmt):
    img = np.broadcast_to(np.array(rgb, np.float32).reshape(1, 3, 1, 1), (1, 3, 2, 2))
    got = YF.rgb_to_yuv420(img, fmt)[0].tolist()
    assert got[0] == got[1] == got[2] == got[3]
    return tuple(got[3:])


@pytest.mark.parametrize("fmt, rgb, yuv", [
    (TEN, (0, 0, 0), (64, 512, 512)), (TEN, (1, 1, 1), (940, 512, 512)), (TEN, (1, 0, 0), (250, 409, 960)),
    ((10, "bt601", False), (1, 0, 0), (326, 361, 960)), ((8, "bt709", False), (1, 0, 0), (63, 102, 240))])
def test_known_answers(fmt, rgb, yuv):
    assert _flat(rgb, fmt) == yuv
    img = torch.tensor(rgb, dtype=torch.float32).view(1, 3, 1, 1).expand(1, 3, 2, 2)
    got = YF.from_bytes(rgb_to_i420(img, fmt=_fmt(fmt)).numpy(), fmt)[0].tolist()
    assert got == [yuv[0]] * 4 + [yuv[1], yuv[2]]


@pytest.mark.parametrize("fmt", YF.ALL_FORMATS, ids=YF.fmt_id)
def test_black_white_grey(fmt):
    P, yoff, coff, ys, _ = YF.spans(fmt)
    assert _flat((0, 0, 0), fmt) == (yoff, coff, coff)
    assert _flat((1, 1, 1), fmt) == (yoff + ys, coff, coff)
    for g in (0.1, 0.25, 0.5, 0.9):
        assert _flat((g, g, g), fmt)[1:] == (coff, coff)
    # the legacy format with exact coefficients is NOT the legacy kernel: red
    if fmt == YF.LEGACY:
        assert _flat((1, 0, 0), fmt)[0] == 81 and Y.rgb_to_i420(np.ones((1, 3, 2, 2), np.float32) *
                                                               np.array([1, 0, 0], np.float32).reshape(1, 3, 1, 1))[0, 0] == 82


@pytest.mark.parametrize("depth", YF.DEPTHS)
def test_quantizer_inverts_the_grid(depth):
    P = 2 ** depth - 1
    k = np.arange(P + 1)
    assert np.array_equal(YF.quantize(k.astype(np.float32) / np.float32(P), P), k)
    x = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 2.0, -1.0], np.float32)
    assert YF.quantize(x, P).tolist() == [0, P, 0, 0, 0, P, P, 0]


@pytest.mark.parametrize("fmt", YF.ALL_FORMATS, ids=YF.fmt_id)
def test_round_trip(fmt):
    """200 000 seeded flat 2x2 blocks, uniform over the legal codes: where the
    inverse does not clip (at least 20 % of them; this draw gives 23.5-24.5 %),
    forward o inverse returns U and V exactly and Y within 1."""
    P, yoff, coff, ys, cs = YF.spans(fmt)
    rng = np.random.default_rng(1)
    n = 200000
    clo, chi = (0, P) if fmt[2] else (coff - cs // 2, coff + cs // 2)
    y, u, v = rng.integers(yoff, yoff + ys + 1, n), rng.integers(clo, chi + 1, n), rng.integers(clo, chi + 1, n)
    # block k at columns 2k, 2k+1 of a 2 x 2n frame
    frame = np.concatenate([np.repeat(y, 2), np.repeat(y, 2), u, v])[None]
    raw = YF.yuv420_to_rgb_int(frame, 2, 2 * n, fmt, clamp=False)[0]
    ok = ((raw >= 0) & (raw <= P)).all(axis=(0, 1))[::2]
    share = ok.mean()
    rgb = YF.yuv420_to_rgb(frame, 2, 2 * n, fmt)
    back = YF.rgb_to_yuv420(rgb, fmt)[0]
    y2, u2, v2 = back[:2 * n:2], back[4 * n:5 * n], back[5 * n:]
    worst = [int(np.abs(a - b)[ok].max()) for a, b in ((y2, y), (u2, u), (v2, v))]
    print(f"{YF.fmt_id(fmt)}: unclipped share {share:.4f}, max errors {worst}")
    assert share >= 0.20
    assert worst[0] <= 1 and worst[1:] == [0, 0]


# --------------------------------------------------------------------------
# the torch dispatch against the numpy statement

@fmt_param
def test_torch_output_equals_numpy(fmt):
    d, P = _fmt(fmt), YF.spans(fmt)[0]
    for h, w in YF.SHAPES:
        for f in YF.FRAMES:
            for kind in YF.CLASSES:
                x = YF.values(kind, f, h, w, P)
                want = YF.rgb_to_yuv420(x, fmt)
                got = rgb_to_i420(torch.from_numpy(x), fmt=d)
                assert got.dtype == torch.uint8 and got.shape == (f, d.frame_bytes(h, w))
                assert np.array_equal(got.numpy(), YF.to_bytes(want, fmt)), (h, w, f, kind)
            ref = YF.reference_samples(f, h, w, fmt)
            got2, sse = rgb_to_i420(torch.from_numpy(x), torch.from_numpy(YF.to_bytes(ref, fmt)), fmt=d)
            assert np.array_equal(got2.numpy(), YF.to_bytes(want, fmt))
            assert sse.dtype == torch.int64 and np.array_equal(sse.numpy(), YF.sse(want, ref, h, w))
            _, zero = rgb_to_i420(torch.from_numpy(x), got2, fmt=d)
            assert not zero.any()


@fmt_param
def test_torch_input_equals_numpy(fmt):
    d = _fmt(fmt)
    for h, w in YF.SHAPES:
        for kind in YF.INPUT_CLASSES:
            s = YF.input_values(kind, 1, h, w, fmt)
            want = YF.yuv420_to_rgb(s, h, w, fmt)
            got = i420_to_rgb(torch.from_numpy(YF.to_bytes(s, fmt)[0].copy()), h, w, d)
            assert got.dtype == torch.float32 and got.shape == (1, 3, h, w)
            assert np.array_equal(got.numpy(), want), (h, w, kind)
            if d.sample_bytes == 2:  # the samples themselves, as int16
                words = torch.from_numpy(s[0].astype(np.uint16).view(np.int16).copy())
                assert np.array_equal(i420_to_rgb(words, h, w, d).numpy(), want)
    with pytest.raises(ValueError):
        i420_to_rgb(torch.zeros(5, dtype=torch.uint8), 2, 2, d)


def test_input_and_output_are_inverse_on_the_grid():
    """What the input conversion writes, k / P, quantizes back to k: a source's
    frame through both conversions comes back within the round trip's bound."""
    s = YF.input_values("legal", 1, 6, 10, TEN)
    rgb = i420_to_rgb(torch.from_numpy(YF.to_bytes(s, TEN)[0].copy()), 6, 10, _fmt(TEN))
    assert np.array_equal(YF.quantize(rgb.numpy(), 1023), YF.yuv420_to_rgb_int(s, 6, 10, TEN))


def test_legacy_format_keeps_its_bytes():
    """No format, and the legacy format by name, are today's conversions."""
    for h, w in ((6, 10), (18, 24)):
        x = Y.values("uniform", 2, h, w)
        want = Y.rgb_to_i420(x)
        t = torch.from_numpy(x)
        assert np.array_equal(rgb_to_i420(t).numpy(), want)
        assert np.array_equal(rgb_to_i420(t, fmt=YuvFormat()).numpy(), want)
        assert np.array_equal(rgb_to_i420(t, None, YuvFormat(8, "bt601", False)).numpy(), want)
        ref = Y.reference_frames(2, h, w)
        _, sse = rgb_to_i420(t, torch.from_numpy(ref), fmt=YuvFormat())
        assert np.array_equal(sse.numpy(), Y.sse(want, ref, h, w))
        raw = torch.from_numpy(ref[0].copy())
        assert torch.equal(i420_to_rgb(raw, h, w), i420_to_rgb(raw, h, w, YuvFormat()))
    # and they are not the exact-coefficient arithmetic: pure red
    red = np.zeros((1, 3, 2, 2), np.float32)
    red[:, 0] = 1
    assert Y.rgb_to_i420(red)[0, 0] == 82 and YF.rgb_to_yuv420(red, YF.LEGACY)[0, 0] == 81


def test_c_entries_argument_errors_without_launch():
    from gsvc_amd import _lib
    lib = _lib.load()
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(65)  # never dereferenced: the argument checks fail first

    def f(*v):
        return (ctypes.c_int * 3)(*v)

    ten, legacy, eight = f(10, 1, 0), f(8, 0, 0), f(8, 1, 0)
    out_cases = [((1, p, 2, 2, legacy, p, None, None), b"legacy"), ((1, p, 2, 2, f(9, 1, 0), p, None, None), b"bit_depth"),
                 ((1, p, 2, 2, f(10, 2, 0), p, None, None), b"matrix"), ((1, p, 2, 2, f(10, 1, 2), p, None, None), b"full_range"),
                 ((1, p, 2, 2, None, p, None, None), b"missing format"),
                 ((0, p, 2, 2, ten, p, None, None), b"frames"), ((1, p, 3, 2, ten, p, None, None), b"even"),
                 ((1, p, 2, 7, ten, p, None, None), b"even"), ((1, p, 0, 2, ten, p, None, None), b"even"),
                 ((1, None, 2, 2, ten, p, None, None), b"missing buffer"), ((1, p, 2, 2, ten, None, None, None), b"missing buffer"),
                 ((1, p, 2, 2, ten, p, p, None), b"sse"), ((1, p, 2, 2, ten, odd, None, None), b"odd address"),
                 ((1, p, 2, 2, ten, p, odd, p), b"odd address"), ((1, p, 2, 2, eight, p, p, None), b"sse")]
    for args, msg in out_cases:
        assert lib.gsvc_rgb_to_yuv420(*args, None) == 1, args
        assert msg in lib.gsvc_last_error(), (args, lib.gsvc_last_error())
    in_cases = [((1, p, 2, 2, legacy, p), b"legacy"), ((1, p, 2, 2, f(9, 1, 0), p), b"bit_depth"),
                ((-1, p, 2, 2, ten, p), b"frames"), ((1, p, 2, 5, ten, p), b"even"), ((1, p, -2, 2, ten, p), b"even"),
                ((1, None, 2, 2, ten, p), b"missing buffer"), ((1, p, 2, 2, ten, None), b"missing buffer"),
                ((1, odd, 2, 2, ten, p), b"odd address")]
    for args, msg in in_cases:
        assert lib.gsvc_yuv420_to_rgb(*args, None) == 1, args
        assert msg in lib.gsvc_last_error(), (args, lib.gsvc_last_error())
    assert lib.gsvc_yuv_format_table(f(9, 0, 0), (ctypes.c_longlong * 18)()) == 1
    assert lib.gsvc_yuv_format_table(ten, None) == 1 and lib.gsvc_yuv_format_table(None, (ctypes.c_longlong * 18)()) == 1
    assert lib.gsvc_abi_version() == 4


# --------------------------------------------------------------------------
# the container

def _gop_cpu(plan=GOP, h=H, w=W, seed=5):
    """As tests/test_yuv_out_cpu.py: frame streams of untrained models on the
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


def test_header_flags(gop, tmp_path):
    streams, _ = gop
    path = tmp_path / "a.gsvf"
    codec.write_video(path, streams)
    plain = path.read_bytes()
    assert struct.unpack_from("<I", plain, 28)[0] == 0 and codec.read_video(path).format == YuvFormat()
    for f in YF.ALL_FORMATS:
        codec.write_video(path, streams, fmt=_fmt(f))
        blob = path.read_bytes()
        assert struct.unpack_from("<II", blob, 4) == (1, H)  # still version 1
        assert struct.unpack_from("<I", blob, 28)[0] == YF.flags(f)
        assert blob[:28] == plain[:28] and blob[32:] == plain[32:]  # nothing else moves
        vid = codec.read_video(path)
        assert vid.format == _fmt(f) and vid.num_frames == len(streams)
    good = bytearray(plain)
    for bit in range(32):
        if bit in (0, 1, 4, 6):
            continue
        struct.pack_into("<I", good, 28, 0x11 | 1 << bit)
        path.write_bytes(bytes(good))
        with pytest.raises(ValueError, match="unknown file flags"):
            codec.read_video(path)
        with pytest.raises(ValueError, match="unknown file flags"):
            codec.decode_video(str(path), device="cpu")


def test_decode_frames_cpu_formats(gop):
    streams, imgs = gop
    d = _fmt(TEN)
    out = C.decode_frames(streams[:3], "cpu", output="i420", fmt=d)
    assert out.shape == (3, d.frame_bytes(H, W))
    assert np.array_equal(out.numpy(), YF.to_bytes(YF.rgb_to_yuv420(imgs[:3], TEN), TEN))
    assert np.array_equal(C.decode_frames(streams[:3], "cpu", output="i420").numpy(), Y.rgb_to_i420(imgs[:3]))
    with pytest.raises(ValueError):
        C.decode_frames(streams[:3], "cpu", fmt=d)  # a format without output="i420"


def test_decode_video_cpu_ten_bit(gop, tmp_path):
    streams, imgs = gop
    d = _fmt(TEN)
    size = d.frame_bytes(H, W)
    want = YF.rgb_to_yuv420(imgs, TEN)
    path = tmp_path / "ten.gsvf"
    codec.write_video(path, streams, fmt=d)
    src = YF.input_values("legal", 5, H, W, TEN, seed=3)
    (tmp_path / "src.yuv").write_bytes(YF.to_bytes(src, TEN).tobytes())
    res = codec.decode_video(str(path), str(tmp_path / "out.yuv"), device="cpu", batch=2,
                             reference=str(tmp_path / "src.yuv"))
    assert res["frames"] == 5 and res["bytes_written"] == 5 * size == 5 * H * W * 3
    assert (tmp_path / "out.yuv").read_bytes() == YF.to_bytes(want, TEN).tobytes()
    e = YF.sse(want, src, H, W)
    for f in range(5):
        p = [YF.psnr(e[f, 0], H * W, 1023), YF.psnr(e[f, 1], H * W // 4, 1023), YF.psnr(e[f, 2], H * W // 4, 1023)]
        assert (res["psnr_y"][f], res["psnr_u"][f], res["psnr_v"][f]) == pytest.approx(p, rel=1e-12)
        assert res["psnr_yuv"][f] == pytest.approx((6 * p[0] + p[1] + p[2]) / 8, rel=1e-12)
    (tmp_path / "same.yuv").write_bytes(YF.to_bytes(want, TEN).tobytes())
    same = codec.decode_video(str(path), device="cpu", reference=str(tmp_path / "same.yuv"))
    assert all(np.isinf(p) for k in ("psnr_y", "psnr_u", "psnr_v", "psnr_yuv") for p in same[k])
    part = codec.decode_video(str(path), str(tmp_path / "part.yuv"), device="cpu", batch=2, frames=range(3, 5))
    assert part["bytes_written"] == 2 * size
    assert (tmp_path / "part.yuv").read_bytes() == YF.to_bytes(want[3:5], TEN).tobytes()
    with pytest.raises(ValueError, match="frames of"):  # an 8-bit source is half as long
        (tmp_path / "short.yuv").write_bytes(bytes(5 * size // 2))
        codec.decode_video(str(path), device="cpu", reference=str(tmp_path / "short.yuv"))
    # fmt= re-targets the output: an 8-bit file to 10 bits, a 10-bit file to the legacy bytes
    codec.write_video(tmp_path / "eight.gsvf", streams)
    r = codec.decode_video(str(tmp_path / "eight.gsvf"), str(tmp_path / "up.yuv"), device="cpu", fmt=d)
    assert r["bytes_written"] == 5 * size
    assert (tmp_path / "up.yuv").read_bytes() == YF.to_bytes(want, TEN).tobytes()
    codec.decode_video(str(tmp_path / "eight.gsvf"), str(tmp_path / "plain.yuv"), device="cpu")
    assert (tmp_path / "plain.yuv").read_bytes() == Y.rgb_to_i420(imgs).tobytes()
    codec.decode_video(str(path), str(tmp_path / "down.yuv"), device="cpu", fmt=YuvFormat())
    assert (tmp_path / "down.yuv").read_bytes() == Y.rgb_to_i420(imgs).tobytes()


# --------------------------------------------------------------------------
# the command lines

def _ten_bit_source(tmp_path, h=32, w=48, frames=3):
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    planes = []
    for f in range(frames):
        y = ((xx * 17 + yy * 11 + 80 * f) % 876 + 64).reshape(-1)
        planes.append(np.concatenate([y, np.full(h * w // 4, 400 + 40 * f), np.full(h * w // 4, 560)]))
    src = np.stack(planes).astype(np.int64)
    (tmp_path / "src.yuv").write_bytes(YF.to_bytes(src, TEN).tobytes())
    return src


def test_load_yuv_frames_ten_bit(tmp_path):
    src = _ten_bit_source(tmp_path)
    frames, total = video.load_yuv_frames(str(tmp_path / "src.yuv"), 48, 32, "cpu", fmt=_fmt(TEN))
    assert total == 3 and sorted(frames) == [0, 1, 2]
    want = YF.yuv420_to_rgb(src, 32, 48, TEN)
    assert all(np.array_equal(frames[i].numpy()[0], want[i]) for i in range(3))
    assert video.load_yuv_frames(str(tmp_path / "src.yuv"), 48, 32, "cpu")[1] == 6  # read as 8-bit: twice as many


def test_cli_encode_info_decode_ten_bit(tmp_path, capsys):
    h, w, frames, n = 32, 48, 3, 40
    _ten_bit_source(tmp_path, h, w, frames)
    g = torch.Generator().manual_seed(11)
    models = {f"frame_{f + 1}": {"_xyz": torch.atanh(1.8 * (torch.rand(n, 2, generator=g) - 0.5)),
                                 "_cholesky": 3.0 * torch.rand(n, 3, generator=g),
                                 "_features_dc": torch.rand(n, 3, generator=g)} for f in range(frames)}
    torch.save(models, tmp_path / "models.pth")
    enc = codec.main(["encode", str(tmp_path / "models.pth"), str(tmp_path / "src.yuv"), str(tmp_path / "v.gsvf"),
                      "--width", str(w), "--height", str(h), "--iterations", "2", "--k_frames", "1,3",
                      "--seed", "3", "--device", "cpu", "--bit_depth", "10", "--matrix", "bt709"])
    assert enc["frames"] == frames
    assert codec.read_video(tmp_path / "v.gsvf").format == _fmt(TEN)
    capsys.readouterr()
    info = codec.main(["info", str(tmp_path / "v.gsvf")])
    assert json.loads(capsys.readouterr().out) == info
    assert info["format"] == {"bit_depth": 10, "matrix": "bt709", "full_range": False}
    size = _fmt(TEN).frame_bytes(h, w)
    dec = codec.main(["decode", str(tmp_path / "v.gsvf"), str(tmp_path / "out.yuv"), "--device", "cpu",
                      "--batch", "2", "--reference", str(tmp_path / "src.yuv")])
    assert (tmp_path / "out.yuv").stat().st_size == frames * size == dec["bytes_written"]
    assert len(dec["psnr_yuv"]) == frames and all(np.isfinite(dec["psnr_yuv"]))
    imgs = C.decode_frames([codec.read_video(tmp_path / "v.gsvf").frame(i) for i in range(frames)], "cpu").numpy()
    assert (tmp_path / "out.yuv").read_bytes() == YF.to_bytes(YF.rgb_to_yuv420(imgs, TEN), TEN).tobytes()
    # the override: the same file as 8-bit bt709 full range (one option leaves the file's others)
    over = codec.main(["decode", str(tmp_path / "v.gsvf"), str(tmp_path / "o8.yuv"), "--device", "cpu",
                       "--bit_depth", "8", "--full_range"])
    f8 = (8, "bt709", True)
    assert over["bytes_written"] == frames * h * w * 3 // 2
    assert (tmp_path / "o8.yuv").read_bytes() == YF.to_bytes(YF.rgb_to_yuv420(imgs, f8), f8).tobytes()


def test_video_cli_takes_a_ten_bit_dataset(tmp_path):
    """python -m gsvc_amd.video --dataset with the three options: the frames it
    trains on are the 10-bit conversion's."""
    src = _ten_bit_source(tmp_path)
    args = video.parse_args(["-d", str(tmp_path / "src.yuv"), "--width", "48", "--height", "32",
                             "--bit_depth", "10", "--matrix", "bt709"])
    fmt = video.format_of_arguments(args)
    assert fmt == _fmt(TEN) and video.format_of_arguments(video.parse_args([])) is None
    assert video.format_of_arguments(video.parse_args(["--full_range"])) == YuvFormat(8, "bt601", True)
    frames, total = video.load_yuv_frames(args.dataset, args.width, args.height, "cpu", [1], fmt=fmt)
    assert total == 3 and np.array_equal(frames[1].numpy()[0], YF.yuv420_to_rgb(src, 32, 48, TEN)[1])
