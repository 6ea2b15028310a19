"""GPU: gsvc_yuv420_to_rgb / gsvc_rgb_to_yuv420 (csrc/yuv_conv.hip) byte for byte
against the numpy statement of their arithmetic (tests/yuv_format_cases.py) on
both layouts, the exact 64-bit SSE, ``decode_frames(output="i420", fmt=...)``,
a 10-bit file through ``decode_video`` on both devices, one 1080p case, and
the legacy call's unchanged output."""
import numpy as np
import pytest
import torch

import yuv_cases as Y
import yuv_format_cases as YF

from gsvc_amd import codec
from gsvc_amd import compress as C
from gsvc_amd.video import YuvFormat, i420_to_rgb, rgb_to_i420

TEN = (10, "bt709", False)
fmt_param = pytest.mark.parametrize("fmt", YF.GPU_FORMATS, ids=YF.fmt_id)
shape_param = pytest.mark.parametrize("shape", YF.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")


def _fmt(f):
    return YuvFormat(*f)


def _offset_bytes(raw, offset, dev):
    """The bytes ``raw`` (numpy uint8, flat) on the device, ``offset`` bytes into a
    16-byte aligned buffer, one guard byte pattern on either side."""
    buf = torch.full((raw.size + offset + 16,), 0xA5, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + raw.size]
    view.copy_(torch.from_numpy(raw))
    return buf, view


def _call_out(x, fmt, out, ref=None, sse=None):
    """The C entry with caller-owned buffers (any alignment)."""
    from gsvc_amd import _lib as L
    f, _, h, w = x.shape
    L.call("gsvc_rgb_to_yuv420", f, L.ptr(x), h, w, _fmt(fmt)._c(), L.ptr(out), L.ptr(ref), L.ptr(sse),
           L.stream(x.device))


def _call_in(raw, f, h, w, fmt, out):
    from gsvc_amd import _lib as L
    L.call("gsvc_yuv420_to_rgb", f, L.ptr(raw), h, w, _fmt(fmt)._c(), L.ptr(out), L.stream(raw.device))


@shape_param
@fmt_param
def test_output_kernel_equals_numpy(cuda, fmt, shape):
    h, w = shape
    d, P = _fmt(fmt), YF.spans(fmt)[0]
    size = d.frame_bytes(h, w)
    for f in YF.FRAMES:
        for kind in YF.CLASSES:
            x = YF.values(kind, f, h, w, P)
            want = YF.to_bytes(YF.rgb_to_yuv420(x, fmt), fmt)
            xd = torch.from_numpy(x).to(cuda)
            got = rgb_to_i420(xd, fmt=d)
            assert got.dtype == torch.uint8 and got.shape == (f, size) and got.data_ptr() % 16 == 0
            assert np.array_equal(got.cpu().numpy(), want), (f, kind)
            # the fallback layout at the same shape: the sample buffer 2 and 8
            # bytes off 16-byte alignment; the guard bytes stay untouched
            for offset in (2, 8):
                buf = torch.full((f * size + offset + 16,), 0xA5, dtype=torch.uint8, device=cuda)
                assert buf.data_ptr() % 16 == 0
                _call_out(xd, fmt, buf[offset:])
                host = buf.cpu().numpy()
                assert (host[:offset] == 0xA5).all() and (host[offset + f * size:] == 0xA5).all()
                assert np.array_equal(host[offset:offset + f * size].reshape(f, size), want), (f, kind, offset)


@shape_param
@fmt_param
def test_input_kernel_equals_numpy(cuda, fmt, shape):
    h, w = shape
    d = _fmt(fmt)
    for f in YF.FRAMES:
        for kind in YF.INPUT_CLASSES:
            s = YF.input_values(kind, f, h, w, fmt)
            want = YF.yuv420_to_rgb(s, h, w, fmt)
            raw = YF.to_bytes(s, fmt)
            rd = torch.from_numpy(raw).to(cuda)
            out = torch.empty((f, 3, h, w), dtype=torch.float32, device=cuda)
            _call_in(rd, f, h, w, fmt, out)  # the whole batch in one launch
            assert np.array_equal(out.cpu().numpy(), want), (f, kind)
            assert np.array_equal(i420_to_rgb(rd[0], h, w, d).cpu().numpy(), want[:1])  # one frame, public call
            for offset in (2, 8):  # the fallback layout
                _, view = _offset_bytes(raw.reshape(-1), offset, cuda)
                out.fill_(-1.0)
                _call_in(view, f, h, w, fmt, out)
                assert np.array_equal(out.cpu().numpy(), want), (f, kind, offset)
    if d.sample_bytes == 2:  # int16 samples, and a view at an odd address (copied by the Python layer)
        words = torch.from_numpy(s[0].astype(np.uint16).view(np.int16).copy()).to(cuda)
        assert np.array_equal(i420_to_rgb(words, h, w, d).cpu().numpy(), want[:1])
        _, view = _offset_bytes(raw[0], 1, cuda)
        assert view.data_ptr() % 2 == 1
        assert np.array_equal(i420_to_rgb(view, h, w, d).cpu().numpy(), want[:1])


@shape_param
@fmt_param
def test_sse_is_exact(cuda, fmt, shape):
    h, w = shape
    d, P = _fmt(fmt), YF.spans(fmt)[0]
    size = d.frame_bytes(h, w)
    for f in YF.FRAMES:
        x = YF.values("uniform", f, h, w, P, seed=1)
        want = YF.rgb_to_yuv420(x, fmt)
        ref = YF.reference_samples(f, h, w, fmt)
        e = YF.sse(want, ref, h, w)
        xd, rd = torch.from_numpy(x).to(cuda), torch.from_numpy(YF.to_bytes(ref, fmt)).to(cuda)
        got, sse = rgb_to_i420(xd, rd, fmt=d)
        assert sse.dtype == torch.int64 and sse.shape == (f, 3)
        assert np.array_equal(got.cpu().numpy(), YF.to_bytes(want, fmt)) and np.array_equal(sse.cpu().numpy(), e)
        _, again = rgb_to_i420(xd, rd, fmt=d)
        assert torch.equal(sse, again)
        _, zero = rgb_to_i420(xd, got, fmt=d)  # the output as its own reference
        assert not zero.any()
        # sse pre-filled with garbage: the entry zeroes it; the fallback layout
        # (reference 2 bytes off) counts the same
        out = torch.empty((f, size), dtype=torch.uint8, device=cuda)
        filled = torch.full((f, 3), -0x123456789, dtype=torch.int64, device=cuda)
        _call_out(xd, fmt, out, rd, filled)
        assert np.array_equal(filled.cpu().numpy(), e)
        _, rview = _offset_bytes(YF.to_bytes(ref, fmt).reshape(-1), 2, cuda)
        filled.fill_(77)
        _call_out(xd, fmt, out, rview, filled)
        assert np.array_equal(filled.cpu().numpy(), e)
        assert np.array_equal(out.cpu().numpy(), YF.to_bytes(want, fmt))


@pytest.mark.parametrize("shape", [(18, 24), (16, 520)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sse_of_extreme_planes_16_bit(cuda, shape):
    """All-0 against all-P planes at 16 bits: every difference squared is
    65535^2, just below 2^32, through the lane, wave and block sums; both ways
    round, both layouts, twice."""
    h, w = shape
    fmt = (16, "bt709", True)
    d = _fmt(fmt)
    n = h * w * 3 // 2
    zeros = np.zeros((2, 3, h, w), np.float32)  # black: (0, 32768, 32768)
    want = YF.rgb_to_yuv420(zeros, fmt)
    ref = np.full((2, n), 65535, np.int64)
    e = YF.sse(want, ref, h, w)
    assert e[0, 0] == h * w * 65535 ** 2
    xd, rd = torch.from_numpy(zeros).to(cuda), torch.from_numpy(YF.to_bytes(ref, fmt)).to(cuda)
    got, sse = rgb_to_i420(xd, rd, fmt=d)
    assert np.array_equal(got.cpu().numpy(), YF.to_bytes(want, fmt)) and np.array_equal(sse.cpu().numpy(), e)
    assert torch.equal(rgb_to_i420(xd, rd, fmt=d)[1], sse)
    # white luma (65535) against all-0 planes, through the fallback layout
    ones = np.ones((2, 3, h, w), np.float32)
    want1 = YF.rgb_to_yuv420(ones, fmt)
    e1 = YF.sse(want1, np.zeros((2, n), np.int64), h, w)
    assert e1[0, 0] == h * w * 65535 ** 2
    _, rview = _offset_bytes(np.zeros(2 * n * 2, np.uint8), 2, cuda)
    out = torch.empty((2, 2 * n), dtype=torch.uint8, device=cuda)
    filled = torch.empty((2, 3), dtype=torch.int64, device=cuda)
    _call_out(torch.from_numpy(ones).to(cuda), fmt, out, rview, filled)
    assert np.array_equal(filled.cpu().numpy(), e1) and np.array_equal(out.cpu().numpy(), YF.to_bytes(want1, fmt))


def test_1080p_ten_bit(cuda):
    h, w, f = 1080, 1920, 2
    d = _fmt(TEN)
    x = YF.values("uniform", f, h, w, 1023)
    want = YF.rgb_to_yuv420(x, TEN)
    ref = YF.reference_samples(f, h, w, TEN)
    got, sse = rgb_to_i420(torch.from_numpy(x).to(cuda), torch.from_numpy(YF.to_bytes(ref, TEN)).to(cuda), fmt=d)
    assert np.array_equal(got.cpu().numpy(), YF.to_bytes(want, TEN))
    assert np.array_equal(sse.cpu().numpy(), YF.sse(want, ref, h, w))
    back = torch.empty((f, 3, h, w), dtype=torch.float32, device=cuda)
    _call_in(got, f, h, w, TEN, back)
    assert np.array_equal(back.cpu().numpy(), YF.yuv420_to_rgb(want, h, w, TEN))


# --------------------------------------------------------------------------
# the legacy calls

def test_calls_without_a_format_are_the_legacy_kernels(cuda):
    from gsvc_amd import _lib as L
    h, w = 18, 24
    raw = torch.from_numpy(Y.reference_frames(1, h, w)[0]).to(cuda)
    want = torch.empty((1, 3, h, w), dtype=torch.float32, device=cuda)
    L.call("gsvc_i420_to_rgb", L.ptr(raw), h, w, L.ptr(want), L.stream(cuda))
    assert torch.equal(i420_to_rgb(raw, h, w), want)
    assert torch.equal(i420_to_rgb(raw, h, w, YuvFormat()), want)
    x = Y.values("uniform", 2, h, w)
    xd = torch.from_numpy(x).to(cuda)
    assert np.array_equal(rgb_to_i420(xd).cpu().numpy(), Y.rgb_to_i420(x))
    assert np.array_equal(rgb_to_i420(xd, fmt=YuvFormat()).cpu().numpy(), Y.rgb_to_i420(x))
    out = torch.empty((2, h * w * 3 // 2), dtype=torch.uint8, device=cuda)
    with pytest.raises(RuntimeError, match="legacy"):  # the new entry refuses the legacy format
        _call_out(xd, YF.LEGACY, out)
    with pytest.raises(RuntimeError, match="legacy"):
        _call_in(raw, 1, h, w, YF.LEGACY, want)


# --------------------------------------------------------------------------
# decode_frames(output="i420", fmt=...) and decode_video

def _gop(h, w, plan):
    """As tests/test_yuv_out_gpu.py: untrained models, every delta on the
    decoded parameters of the frame before it; versions alternate."""
    torch.manual_seed(5)
    kw = dict(H=h, W=w, BLOCK_H=16, BLOCK_W=16, device="cuda", lr=1e-3, quantize=True, opt_type="adan")
    streams, state = [], None
    for k, (n, key) in enumerate(plan):
        if key:
            m = C.GaussianVideoFrameQ(num_points=n, **kw).cuda()
            with torch.no_grad():
                m._cholesky.mul_(3.0)
            state = None
        else:
            m = C.GaussianVideoDelta(num_points=n, **kw).cuda()
            with torch.no_grad():
                m._xyz.copy_(0.05 * torch.randn(n, 2))
                m._cholesky.copy_(0.3 * torch.randn(n, 3))
                m._features_dc.copy_(0.1 * torch.randn(n, 3))
                m.p_xyz.copy_(state[0][:n])
                m.p_cholesky.copy_(state[1][:n])
                m.p_features_dc.copy_(state[2][:n])
        m._init_data()
        m.eval()
        s = C.encode_frame(m, entropy=bool(k & 1))
        xq, _, cq, Lpre, _, _ = C.unpack_frames([s], "cuda", prev=state)
        state = (xq, Lpre, cq)
        streams.append(s)
    return streams


@pytest.mark.parametrize("hw", [(48, 64), (50, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_decode_frames_ten_bit(cuda, hw):
    h, w = hw
    d = _fmt(TEN)
    streams = _gop(h, w, [(257, True), (200, False), (65, False)])
    imgs, st = C.decode_frames(streams, "cuda", return_state=True)
    want = YF.rgb_to_yuv420(imgs.cpu().numpy(), TEN)
    out, st2 = C.decode_frames(streams, "cuda", return_state=True, output="i420", fmt=d)
    assert out.dtype == torch.uint8 and out.shape == (3, d.frame_bytes(h, w))
    assert np.array_equal(out.cpu().numpy(), YF.to_bytes(want, TEN))
    assert all(torch.equal(a, b) for a, b in zip(st, st2))
    src = YF.reference_samples(3, h, w, TEN)
    out2, sse = C.decode_frames(streams, "cuda", output="i420", fmt=d,
                                reference=torch.from_numpy(YF.to_bytes(src, TEN)).to(cuda))
    assert np.array_equal(out2.cpu().numpy(), YF.to_bytes(want, TEN))
    assert np.array_equal(sse.cpu().numpy(), YF.sse(want, src, h, w))


def test_a_ten_bit_file_decodes_alike_on_both_devices(cuda, tmp_path):
    h, w = 48, 64
    d = _fmt(TEN)
    size = d.frame_bytes(h, w)
    plan = [(257, True), (200, False), (65, False), (129, True), (100, False)]
    streams = _gop(h, w, plan)
    path = tmp_path / "v.gsvf"
    codec.write_video(path, streams, fmt=d)
    assert codec.read_video(path).format == d
    src = YF.input_values("legal", 5, h, w, TEN, seed=2)
    (tmp_path / "src.yuv").write_bytes(YF.to_bytes(src, TEN).tobytes())
    want = YF.rgb_to_yuv420(C.decode_frames(streams, "cuda").cpu().numpy(), TEN)
    res = codec.decode_video(str(path), str(tmp_path / "gpu.yuv"), batch=2, reference=str(tmp_path / "src.yuv"))
    gpu = (tmp_path / "gpu.yuv").read_bytes()
    assert res["bytes_written"] == 5 * size == len(gpu) and gpu == YF.to_bytes(want, TEN).tobytes()
    e = YF.sse(want, src, h, w)
    for f in range(5):
        p = (YF.psnr(e[f, 0], h * w, 1023), YF.psnr(e[f, 1], h * w // 4, 1023), YF.psnr(e[f, 2], h * w // 4, 1023))
        assert (res["psnr_y"][f], res["psnr_u"][f], res["psnr_v"][f]) == pytest.approx(p, rel=1e-12)
    # the CPU decoder's file: the same bytes
    codec.decode_video(str(path), str(tmp_path / "cpu.yuv"), device="cpu", batch=8)
    a = YF.from_bytes(np.frombuffer((tmp_path / "cpu.yuv").read_bytes(), np.uint8)[None], TEN)
    b = YF.from_bytes(np.frombuffer(gpu, np.uint8)[None], TEN)
    diff = np.abs(a - b)
    print(f"CPU / GPU decoders: {int((diff != 0).sum())} of {diff.size} samples differ, max {int(diff.max())}")
    assert (tmp_path / "cpu.yuv").read_bytes() == gpu
    # the 8-bit override of the same file is the legacy kernel's output
    codec.decode_video(str(path), str(tmp_path / "g8.yuv"), batch=3, fmt=YuvFormat())
    assert (tmp_path / "g8.yuv").read_bytes() == Y.rgb_to_i420(C.decode_frames(streams, "cuda").cpu().numpy()).tobytes()


def test_video_command_line_trains_on_a_ten_bit_dataset(cuda, tmp_path):
    """python -m gsvc_amd.video --dataset with the three options: three 10-bit
    32x48 frames (read as 8-bit the file would hold six), a few iterations each."""
    from gsvc_amd import video as V
    h, w = 32, 48
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    planes = []
    for f in range(3):
        y = ((xx * 17 + yy * 11 + 80 * f) % 876 + 64).reshape(-1)
        planes.append(np.concatenate([y, np.full(h * w // 4, 400 + 40 * f), np.full(h * w // 4, 560)]))
    (tmp_path / "src.yuv").write_bytes(YF.to_bytes(np.stack(planes).astype(np.int64), TEN).tobytes())
    res = V.main(["-d", str(tmp_path / "src.yuv"), "--width", str(w), "--height", str(h), "--bit_depth", "10",
                  "--matrix", "bt709", "--num_points", "60", "--iterations", "30", "--k_frames", "1",
                  "--root", str(tmp_path)])
    assert [r["frame"] for r in res["frames"]] == [1, 2, 3]
    assert all(np.isfinite(r["psnr"]) and r["psnr"] > 0 for r in res["frames"])
