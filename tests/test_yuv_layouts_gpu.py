"""GPU: gsvc_yuv_to_rgb / gsvc_rgb_to_yuv (csrc/yuv_conv.hip) byte for byte
against the numpy statement of their arithmetic (tests/yuv_layout_cases.py) in
the five layouts beyond planar 4:2:0, on the vector and the fallback layout of
the work, the exact 64-bit SSE, ``decode_frames(output="yuv", fmt=...)``, a
p010le file through ``decode_video`` on both devices, two 1080p cases, and the
unchanged output of the calls that name no layout."""
import numpy as np
import pytest
import torch

import yuv_cases as Y
import yuv_format_cases as YF
import yuv_layout_cases as YL

from gsvc_amd import codec
from gsvc_amd import compress as C
from gsvc_amd.video import YuvFormat, i420_to_rgb, rgb_to_i420

TEN = (10, "bt709", False)
# layout x colour triple x shape, without the shapes that break the layout's constraint
CASES = [pytest.param(lay, fmt, shape, id=f"{YL.lay_id(lay)}-{YF.fmt_id(fmt)}-{shape[0]}x{shape[1]}")
         for lay in YL.NEW_LAYOUTS for fmt in YL.GPU_FORMATS for shape in YL.SHAPES if YL.fits(lay, *shape)]
case_param = pytest.mark.parametrize("lay, fmt, shape", CASES)


def _fmt(f, lay=YL.PLANAR420):
    return YuvFormat(f[0], f[1], f[2], lay[0], lay[1])


def _offset_bytes(raw, offset, dev):
    """The bytes ``raw`` (numpy uint8, flat) on the device, ``offset`` bytes into a
    16-byte aligned buffer, one guard byte pattern on either side."""
    buf = torch.full((raw.size + offset + 16,), 0xA5, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + raw.size]
    view.copy_(torch.from_numpy(raw))
    return buf, view


def _call_out(x, fmt, lay, out, ref=None, sse=None):
    """The C entry with caller-owned buffers (any alignment)."""
    from gsvc_amd import _lib as L
    f, _, h, w = x.shape
    L.call("gsvc_rgb_to_yuv", f, L.ptr(x), h, w, _fmt(fmt)._c(), int(lay[0]), int(lay[1] == "semi"), L.ptr(out),
           L.ptr(ref), L.ptr(sse), L.stream(x.device))


def _call_in(raw, f, h, w, fmt, lay, out):
    from gsvc_amd import _lib as L
    L.call("gsvc_yuv_to_rgb", f, L.ptr(raw), h, w, _fmt(fmt)._c(), int(lay[0]), int(lay[1] == "semi"), L.ptr(out),
           L.stream(raw.device))


@case_param
def test_output_kernel_equals_numpy(cuda, lay, fmt, shape):
    h, w = shape
    d, P = _fmt(fmt, lay), YF.spans(fmt)[0]
    size = d.frame_bytes(h, w)
    for f in YL.FRAMES:
        for kind in YF.CLASSES:
            x = YL.values(kind, f, h, w, P)
            want = YL.to_bytes(YL.rgb_to_yuv(x, fmt, lay), fmt)
            xd = torch.from_numpy(x).to(cuda)
            got = rgb_to_i420(xd, fmt=d)
            assert got.dtype == torch.uint8 and got.shape == (f, size) and got.data_ptr() % 16 == 0
            assert np.array_equal(got.cpu().numpy(), want), (f, kind)
            # the fallback layout at the same shape: the sample buffer 2 and 8
            # bytes off 16-byte alignment; the guard bytes stay untouched
            for offset in (2, 8):
                buf = torch.full((f * size + offset + 16,), 0xA5, dtype=torch.uint8, device=cuda)
                assert buf.data_ptr() % 16 == 0
                _call_out(xd, fmt, lay, buf[offset:])
                host = buf.cpu().numpy()
                assert (host[:offset] == 0xA5).all() and (host[offset + f * size:] == 0xA5).all()
                assert np.array_equal(host[offset:offset + f * size].reshape(f, size), want), (f, kind, offset)


@case_param
def test_input_kernel_equals_numpy(cuda, lay, fmt, shape):
    h, w = shape
    d = _fmt(fmt, lay)
    for f in YL.FRAMES:
        for kind in YL.input_classes(fmt, lay):
            s = YL.input_values(kind, f, h, w, fmt, lay)
            want = YL.yuv_to_rgb(s, h, w, fmt, lay)
            raw = YL.to_bytes(s, fmt)
            rd = torch.from_numpy(raw).to(cuda)
            out = torch.empty((f, 3, h, w), dtype=torch.float32, device=cuda)
            _call_in(rd, f, h, w, fmt, lay, out)  # the whole batch in one launch
            assert np.array_equal(out.cpu().numpy(), want), (f, kind)
            assert np.array_equal(i420_to_rgb(rd[0], h, w, d).cpu().numpy(), want[:1])  # one frame, public call
            for offset in (2, 8):  # the fallback layout
                buf, view = _offset_bytes(raw.reshape(-1), offset, cuda)
                out.fill_(-1.0)
                _call_in(view, f, h, w, fmt, lay, out)
                assert np.array_equal(out.cpu().numpy(), want), (f, kind, offset)
                host = buf.cpu().numpy()
                assert (host[:offset] == 0xA5).all() and (host[offset + raw.size:] == 0xA5).all()
    if d.sample_bytes == 2:  # int16 samples, and a view at an odd address (copied by the Python layer)
        words = torch.from_numpy(s[0].astype(np.uint16).view(np.int16).copy()).to(cuda)
        assert np.array_equal(i420_to_rgb(words, h, w, d).cpu().numpy(), want[:1])
        _, view = _offset_bytes(raw[0], 1, cuda)
        assert view.data_ptr() % 2 == 1
        assert np.array_equal(i420_to_rgb(view, h, w, d).cpu().numpy(), want[:1])


@case_param
def test_sse_is_exact(cuda, lay, fmt, shape):
    h, w = shape
    d, P = _fmt(fmt, lay), YF.spans(fmt)[0]
    size = d.frame_bytes(h, w)
    for f in YL.FRAMES:
        x = YL.values("uniform", f, h, w, P, seed=1)
        want = YL.rgb_to_yuv(x, fmt, lay)
        ref = YL.reference_words(f, h, w, fmt, lay)
        e = YL.sse(want, ref, h, w, fmt, lay)
        xd, rd = torch.from_numpy(x).to(cuda), torch.from_numpy(YL.to_bytes(ref, fmt)).to(cuda)
        got, sse = rgb_to_i420(xd, rd, fmt=d)
        assert sse.dtype == torch.int64 and sse.shape == (f, 3)
        assert np.array_equal(got.cpu().numpy(), YL.to_bytes(want, fmt)) and np.array_equal(sse.cpu().numpy(), e)
        _, again = rgb_to_i420(xd, rd, fmt=d)
        assert torch.equal(sse, again)
        _, zero = rgb_to_i420(xd, got, fmt=d)  # the output as its own reference
        assert not zero.any()
        # sse pre-filled with garbage: the entry zeroes it; the fallback layout
        # (reference 2 bytes off) counts the same
        out = torch.empty((f, size), dtype=torch.uint8, device=cuda)
        filled = torch.full((f, 3), -0x123456789, dtype=torch.int64, device=cuda)
        _call_out(xd, fmt, lay, out, rd, filled)
        assert np.array_equal(filled.cpu().numpy(), e)
        _, rview = _offset_bytes(YL.to_bytes(ref, fmt).reshape(-1), 2, cuda)
        filled.fill_(77)
        _call_out(xd, fmt, lay, out, rview, filled)
        assert np.array_equal(filled.cpu().numpy(), e)
        assert np.array_equal(out.cpu().numpy(), YL.to_bytes(want, fmt))


@pytest.mark.parametrize("fmt", YL.GPU_FORMATS, ids=YF.fmt_id)
def test_semi_planar_420_is_a_permutation_of_the_existing_kernels_output(cuda, fmt):
    """nv12 / p010 of an image: the bytes the planar 4:2:0 kernels of before
    write for it, re-laid; and nv12 in gives their floats."""
    lay = ("420", "semi")
    for h, w in ((6, 10), (18, 24)):
        P = YF.spans(fmt)[0]
        x = YF.values("uniform", 2, h, w, P)
        xd = torch.from_numpy(x).to(cuda)
        planar = YF.from_bytes(rgb_to_i420(xd, fmt=_fmt(fmt)).cpu().numpy(), fmt)  # today's kernel
        want = YL.to_bytes(YL.i420_to_layout(planar, h, w, fmt, lay), fmt)
        assert np.array_equal(rgb_to_i420(xd, fmt=_fmt(fmt, lay)).cpu().numpy(), want)
        s = YF.input_values("garbage", 1, h, w, fmt) & (P if fmt[0] > 8 else 255)
        semi = YL.to_bytes(YL.i420_to_layout(s, h, w, fmt, lay), fmt)[0]
        today = i420_to_rgb(torch.from_numpy(YF.to_bytes(s, fmt)[0].copy()).to(cuda), h, w, _fmt(fmt))
        assert torch.equal(i420_to_rgb(torch.from_numpy(semi.copy()).to(cuda), h, w, _fmt(fmt, lay)), today)


@pytest.mark.parametrize("name", ["p010le", "yuv444p10le"])
def test_1080p(cuda, name):
    h, w, f = 1080, 1920, 2
    d = YuvFormat.from_pix_fmt(name, "bt709")
    lay = (d.chroma, d.layout)
    x = YL.values("uniform", f, h, w, 1023)
    want = YL.rgb_to_yuv(x, TEN, lay)
    ref = YL.reference_words(f, h, w, TEN, lay)
    got, sse = rgb_to_i420(torch.from_numpy(x).to(cuda), torch.from_numpy(YL.to_bytes(ref, TEN)).to(cuda), fmt=d)
    assert np.array_equal(got.cpu().numpy(), YL.to_bytes(want, TEN))
    assert np.array_equal(sse.cpu().numpy(), YL.sse(want, ref, h, w, TEN, lay))
    back = torch.empty((f, 3, h, w), dtype=torch.float32, device=cuda)
    _call_in(got, f, h, w, TEN, lay, back)
    assert np.array_equal(back.cpu().numpy(), YL.yuv_to_rgb(want, h, w, TEN, lay))


# --------------------------------------------------------------------------
# the calls that name no layout

def test_calls_without_a_layout_are_the_existing_kernels(cuda):
    from gsvc_amd import _lib as L
    h, w = 18, 24
    raw = torch.from_numpy(Y.reference_frames(1, h, w)[0]).to(cuda)
    want = torch.empty((1, 3, h, w), dtype=torch.float32, device=cuda)
    L.call("gsvc_i420_to_rgb", L.ptr(raw), h, w, L.ptr(want), L.stream(cuda))
    assert torch.equal(i420_to_rgb(raw, h, w), want)
    assert torch.equal(i420_to_rgb(raw, h, w, YuvFormat(8, "bt601", False, "420", "planar")), want)
    x = Y.values("uniform", 2, h, w)
    xd = torch.from_numpy(x).to(cuda)
    assert np.array_equal(rgb_to_i420(xd).cpu().numpy(), Y.rgb_to_i420(x))
    assert np.array_equal(rgb_to_i420(xd, fmt=YuvFormat(chroma="420", layout="planar")).cpu().numpy(), Y.rgb_to_i420(x))
    x10 = YF.values("uniform", 2, h, w, 1023)
    out10 = torch.empty((2, h * w * 3), dtype=torch.uint8, device=cuda)
    L.call("gsvc_rgb_to_yuv420", 2, L.ptr(torch.from_numpy(x10).to(cuda)), h, w, _fmt(TEN)._c(), L.ptr(out10), None,
           None, L.stream(cuda))
    assert torch.equal(rgb_to_i420(torch.from_numpy(x10).to(cuda), fmt=YuvFormat(*TEN)), out10)
    assert np.array_equal(out10.cpu().numpy(), YF.to_bytes(YF.rgb_to_yuv420(x10, TEN), TEN))
    out = torch.empty((2, h * w * 3 // 2), dtype=torch.uint8, device=cuda)
    with pytest.raises(RuntimeError, match="planar 4:2:0"):  # the new entries refuse that layout
        _call_out(xd, YF.LEGACY, YL.PLANAR420, out)
    with pytest.raises(RuntimeError, match="planar 4:2:0"):
        _call_in(raw, 1, h, w, TEN, YL.PLANAR420, want)


# --------------------------------------------------------------------------
# decode_frames(output="yuv", fmt=...) and decode_video

def _gop(h, w, plan):
    """As tests/test_yuv_formats_gpu.py: untrained models, every delta on the
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
def test_decode_frames_layouts(cuda, hw):
    h, w = hw
    streams = _gop(h, w, [(257, True), (200, False), (65, False)])
    imgs, st = C.decode_frames(streams, "cuda", return_state=True)
    host = imgs.cpu().numpy()
    for name, fmt in (("nv12", YF.LEGACY), ("yuv422p10le", TEN), ("yuv444p", (8, "bt709", False))):
        d = YuvFormat.from_pix_fmt(name, fmt[1], fmt[2])
        lay = (d.chroma, d.layout)
        want = YL.rgb_to_yuv(host, fmt, lay)
        out, st2 = C.decode_frames(streams, "cuda", return_state=True, output="yuv", fmt=d)
        assert out.dtype == torch.uint8 and out.shape == (3, d.frame_bytes(h, w))
        assert np.array_equal(out.cpu().numpy(), YL.to_bytes(want, fmt)), name
        assert all(torch.equal(a, b) for a, b in zip(st, st2))
        src = YL.reference_words(3, h, w, fmt, lay)
        out2, sse = C.decode_frames(streams, "cuda", output="yuv", fmt=d,
                                    reference=torch.from_numpy(YL.to_bytes(src, fmt)).to(cuda))
        assert np.array_equal(out2.cpu().numpy(), YL.to_bytes(want, fmt))
        assert np.array_equal(sse.cpu().numpy(), YL.sse(want, src, h, w, fmt, lay))


def test_a_p010_file_decodes_alike_on_both_devices(cuda, tmp_path):
    h, w = 48, 64
    lay = ("420", "semi")
    d = _fmt(TEN, lay)
    assert d.pix_fmt == "p010le"
    size = d.frame_bytes(h, w)
    plan = [(257, True), (200, False), (65, False), (129, True), (100, False)]
    streams = _gop(h, w, plan)
    path = tmp_path / "v.gsvf"
    codec.write_video(path, streams, fmt=d)
    assert codec.read_video(path).format == d
    src = YL.input_values("low_bits", 5, h, w, TEN, lay, seed=2)
    (tmp_path / "src.yuv").write_bytes(YL.to_bytes(src, TEN).tobytes())
    want = YL.rgb_to_yuv(C.decode_frames(streams, "cuda").cpu().numpy(), TEN, lay)
    res = codec.decode_video(str(path), str(tmp_path / "gpu.yuv"), batch=2, reference=str(tmp_path / "src.yuv"))
    gpu = (tmp_path / "gpu.yuv").read_bytes()
    assert res["bytes_written"] == 5 * size == len(gpu) and gpu == YL.to_bytes(want, TEN).tobytes()
    e = YL.sse(want, src, h, w, TEN, lay)
    counts = YL.psnr_counts(lay, h, w)
    for f in range(5):
        p = tuple(YF.psnr(e[f, k], counts[k], 1023) for k in range(3))
        assert (res["psnr_y"][f], res["psnr_u"][f], res["psnr_v"][f]) == pytest.approx(p, rel=1e-12)
    # the CPU decoder's file: the same bytes
    codec.decode_video(str(path), str(tmp_path / "cpu.yuv"), device="cpu", batch=8)
    assert (tmp_path / "cpu.yuv").read_bytes() == gpu
    # the same file without a layout is the planar kernel's output
    codec.decode_video(str(path), str(tmp_path / "p.yuv"), batch=3, fmt=_fmt(TEN))
    assert (tmp_path / "p.yuv").read_bytes() == YF.to_bytes(
        YF.rgb_to_yuv420(C.decode_frames(streams, "cuda").cpu().numpy(), TEN), TEN).tobytes()
