"""GPU: gsvc_rgb_to_i420 (csrc/yuv_conv.hip) bit-exact against the numpy
statement of its arithmetic (tests/yuv_cases.py) on both layouts, its exact
integer SSE, ``decode_frames(output="i420")`` and ``decode_video`` from a file
(batches that cut GOPs, the two pinned buffers reused, frame ranges, PSNR);
the entry's 8-byte alignment rule and a partial last block."""
import numpy as np
import pytest
import torch

import yuv_cases as Y

from gsvc_amd import codec
from gsvc_amd import compress as C
from gsvc_amd.video import rgb_to_i420


def _misaligned_input(x, dev):
    """The same values behind a one-float offset: no 16-byte alignment."""
    buf = torch.empty(x.size + 1, dtype=torch.float32, device=dev)
    view = buf[1:].view(x.shape)
    view.copy_(torch.from_numpy(x))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _call(x, out, ref=None, sse=None):
    """The C entry with caller-owned buffers (any alignment)."""
    from gsvc_amd import _lib as L
    f, _, h, w = x.shape
    L.call("gsvc_rgb_to_i420", f, L.ptr(x), h, w, L.ptr(out), L.ptr(ref), L.ptr(sse), L.stream(x.device))


@pytest.mark.parametrize("kind", Y.CLASSES)
@pytest.mark.parametrize("shape", Y.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_numpy(cuda, shape, kind):
    h, w = shape
    size = h * w * 3 // 2
    for f in Y.FRAMES:
        x = Y.values(kind, f, h, w)
        want = Y.rgb_to_i420(x)
        xd = torch.from_numpy(x).to(cuda)
        assert xd.data_ptr() % 16 == 0
        got = rgb_to_i420(xd)
        assert got.dtype == torch.uint8 and got.shape == (f, size) and got.data_ptr() % 8 == 0
        assert np.array_equal(got.cpu().numpy(), want)
        # the bytewise layout at the same shape: an input one float off 16-byte
        # alignment, then an output one byte off; guard bytes stay untouched
        assert np.array_equal(rgb_to_i420(_misaligned_input(x, cuda)).cpu().numpy(), want)
        buf = torch.full((f * size + 2,), 0xA5, dtype=torch.uint8, device=cuda)
        _call(xd, buf[1:])
        host = buf.cpu().numpy()
        assert host[0] == 0xA5 and host[-1] == 0xA5
        assert np.array_equal(host[1:-1].reshape(f, size), want)


def test_input_forms(cuda):
    x = Y.values("uniform", 2, 18, 24)
    want = Y.rgb_to_i420(x)
    t = torch.from_numpy(x).to(cuda)
    assert np.array_equal(rgb_to_i420(t[0]).cpu().numpy(), want[:1])
    hwc = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not hwc.is_contiguous() and np.array_equal(rgb_to_i420(hwc).cpu().numpy(), want)
    assert np.array_equal(rgb_to_i420(t.double()).cpu().numpy(), want)
    with pytest.raises(ValueError):
        rgb_to_i420(t, torch.zeros(3, dtype=torch.uint8, device=cuda))


@pytest.mark.parametrize("shape", Y.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sse_is_exact(cuda, shape):
    h, w = shape
    size = h * w * 3 // 2
    for f in Y.FRAMES:
        x = Y.values("uniform", f, h, w, seed=1)
        want = Y.rgb_to_i420(x)
        ref = Y.reference_frames(f, h, w)
        e = Y.sse(want, ref, h, w)
        xd, rd = torch.from_numpy(x).to(cuda), torch.from_numpy(ref).to(cuda)
        got, sse = rgb_to_i420(xd, rd)
        assert sse.dtype == torch.int64 and sse.shape == (f, 3)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(sse.cpu().numpy(), e)
        _, again = rgb_to_i420(xd, rd)
        assert torch.equal(sse, again)
        _, zero = rgb_to_i420(xd, got)  # the output as its own reference
        assert not zero.any()
        # sse pre-filled with garbage: the entry zeroes it; the bytewise layout
        # (reference one byte off) counts the same
        out = torch.empty((f, size), dtype=torch.uint8, device=cuda)
        filled = torch.full((f, 3), -0x123456789, dtype=torch.int64, device=cuda)
        _call(xd, out, rd, filled)
        assert np.array_equal(filled.cpu().numpy(), e)
        rbuf = torch.empty(f * size + 1, dtype=torch.uint8, device=cuda)
        rbuf[1:].copy_(rd.view(-1))
        filled.fill_(77)
        _call(xd, out, rbuf[1:], filled)
        assert np.array_equal(filled.cpu().numpy(), e) and np.array_equal(out.cpu().numpy(), want)


def test_sse_of_extreme_planes(cuda):
    """Black frames (16, 128, 128) against bytes of 255: every lane carries a
    large sum, through the wave and block reductions of 4 blocks per frame."""
    h, w = 64, 128
    x = torch.zeros((2, 3, h, w), device=cuda)
    ref = torch.full((2, h * w * 3 // 2), 255, dtype=torch.uint8, device=cuda)
    got, sse = rgb_to_i420(x, ref)
    want = Y.rgb_to_i420(np.zeros((2, 3, h, w), np.float32))
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(sse.cpu().numpy(), Y.sse(want, ref.cpu().numpy(), h, w))


# --------------------------------------------------------------------------
# the entry's own alignment rule: rgb 16-byte, out and ref 8-byte (every other
# conversion entry asks 16 of its sample buffers; the rule is an argument of
# the code they share)

def _guarded(nbytes, offset, dev, fill=None):
    """``nbytes`` at ``offset`` into a 16-byte aligned allocation of 0xA5 bytes."""
    buf = torch.full((offset + nbytes + 16,), 0xA5, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + nbytes]
    if fill is not None:
        view.copy_(torch.from_numpy(fill).to(dev).view(-1))
    return buf, view


def _guards_intact(buf, offset, nbytes):
    host = buf.cpu().numpy()
    return bool((host[:offset] == 0xA5).all() and (host[offset + nbytes:] == 0xA5).all())


def _check_offsets(cuda, f, h, w, kind, offsets):
    size = h * w * 3 // 2
    x = Y.values(kind, f, h, w, seed=3)
    want = Y.rgb_to_i420(x)
    ref = Y.reference_frames(f, h, w, seed=3)
    e = Y.sse(want, ref, h, w)
    xd = torch.from_numpy(x).to(cuda)
    assert xd.data_ptr() % 16 == 0
    for off in offsets:
        for with_ref in (False, True):
            buf, out = _guarded(f * size, off, cuda)
            assert out.data_ptr() % 16 == off
            if with_ref:
                rbuf, rd = _guarded(f * size, off, cuda, fill=ref)
                sse = torch.full((f, 3), -0x123456789, dtype=torch.int64, device=cuda)
                _call(xd, out, rd, sse)
                assert np.array_equal(sse.cpu().numpy(), e), (h, w, f, kind, off)
                assert _guards_intact(rbuf, off, f * size) and np.array_equal(rd.cpu().numpy().reshape(f, size), ref)
            else:
                _call(xd, out)
            assert np.array_equal(out.cpu().numpy().reshape(f, size), want), (h, w, f, kind, off, with_ref)
            assert _guards_intact(buf, off, f * size), (h, w, f, kind, off, with_ref)


@pytest.mark.parametrize("shape", [(4, 8), (2, 16), (18, 24), (16, 520)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_out_and_ref_at_8_and_4_byte_offsets(cuda, shape):
    """Offset 8 takes the vector layout (W % 8 == 0, rgb 16-byte, out and ref
    8-byte aligned), offset 4 the bytewise one; same bytes, same sums, nothing
    written outside."""
    h, w = shape
    if shape == (18, 24):  # the case the 8-byte rule exists for: frame 1 starts 8 mod 16
        assert h * w * 3 // 2 == 648 and 648 % 16 == 8
    for f in Y.FRAMES:
        for kind in ("uniform", "special"):
            _check_offsets(cuda, f, h, w, kind, (8, 4))


def test_partial_last_block_of_the_bytewise_layout(cuda):
    """34x258: W % 8 = 2, so one lane per 2x2 block: 2193 units are 8 blocks of
    256 and one of 145, and there is no stride loop to hide behind."""
    h, w = 34, 258
    assert w % 8 == 2 and (h // 2) * (w // 2) == 2193 == 8 * 256 + 145
    _check_offsets(cuda, 2, h, w, "uniform", (0,))


# --------------------------------------------------------------------------
# decode_frames(output="i420") and decode_video

def _gop(h, w, plan):
    """As test_quantize_gpu's _gop: untrained models, every delta on the
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
def test_decode_frames_i420(cuda, hw):
    from gsvc_amd.render import render_frames_sum
    h, w = hw
    streams = _gop(h, w, [(257, True), (200, False), (65, False)])
    imgs, st = C.decode_frames(streams, "cuda", return_state=True)
    # the default call is what it was: render_frames_sum of the unpacked frames
    xq, Lq, cq, _, sizes, _ = C.unpack_frames(streams, "cuda")
    assert sizes == [257, 200, 65]
    ref = render_frames_sum(xq, Lq, cq, sizes, h, w, torch.ones(3, device="cuda"), xyz_tanh=True,
                            cholesky_bound=None)
    assert imgs.dtype == torch.float32 and imgs.shape == (3, 3, h, w) and torch.equal(imgs, ref)
    assert torch.equal(C.decode_frames(streams, "cuda"), imgs)
    want = Y.rgb_to_i420(imgs.cpu().numpy())
    out, st2 = C.decode_frames(streams, "cuda", return_state=True, output="i420")
    assert out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), want)
    assert all(torch.equal(a, b) for a, b in zip(st, st2))
    src = Y.reference_frames(3, h, w)
    (out2, sse) = C.decode_frames(streams, "cuda", output="i420", reference=torch.from_numpy(src).to(cuda))
    assert np.array_equal(out2.cpu().numpy(), want)
    assert np.array_equal(sse.cpu().numpy(), Y.sse(want, src, h, w))


def test_decode_video_from_a_file(cuda, tmp_path):
    h, w, size = 48, 64, 48 * 64 * 3 // 2
    plan = [(257, True), (200, False), (65, False), (129, True), (129, False), (100, False), (31, False)]
    streams = _gop(h, w, plan)
    path = tmp_path / "v.gsvf"
    codec.write_video(path, streams)
    assert codec.read_video(path).key_frames == [0, 3]  # frames 1 and 4, counted from 1
    src = Y.reference_frames(7, h, w, seed=2)
    (tmp_path / "src.yuv").write_bytes(src.tobytes())
    want = Y.rgb_to_i420(C.decode_frames(streams, "cuda").cpu().numpy())

    r8 = codec.decode_video(str(path), str(tmp_path / "b8.yuv"), batch=8, reference=str(tmp_path / "src.yuv"))
    b8 = (tmp_path / "b8.yuv").read_bytes()
    assert r8["frames"] == 7 and r8["bytes_written"] == 7 * size == len(b8) and r8["seconds"] > 0
    assert b8 == want.tobytes()
    # batch = 2 cuts inside both GOPs and fills each pinned buffer twice
    r2 = codec.decode_video(str(path), str(tmp_path / "b2.yuv"), batch=2, reference=str(tmp_path / "src.yuv"))
    assert (tmp_path / "b2.yuv").read_bytes() == b8
    r3 = codec.decode_video(list(streams), str(tmp_path / "b3.yuv"), batch=3)
    assert (tmp_path / "b3.yuv").read_bytes() == b8 and "psnr_y" not in r3

    # the CPU decoder's file: the render's CPU/GPU bar (images within 1e-5,
    # tests/test_cpu_path.py) is at most one quantizer step, so +-1 per byte
    codec.decode_video(str(path), str(tmp_path / "cpu.yuv"), device="cpu", batch=8)
    cpu = np.frombuffer((tmp_path / "cpu.yuv").read_bytes(), np.uint8).astype(np.int64)
    d = np.abs(cpu - np.frombuffer(b8, np.uint8).astype(np.int64))
    print(f"CPU / GPU decoders: {int((d != 0).sum())} of {d.size} bytes differ, max {int(d.max())}")
    assert d.max() <= 1

    for a, b in ((4, 6), (5, 7)):
        r = codec.decode_video(str(path), str(tmp_path / "part.yuv"), batch=2, frames=range(a, b))
        assert r["frames"] == 2 and r["bytes_written"] == 2 * size
        assert (tmp_path / "part.yuv").read_bytes() == b8[a * size:b * size]

    e = Y.sse(want, src, h, w)
    for res in (r8, r2):
        for f in range(7):
            p = (Y.psnr(e[f, 0], h * w), Y.psnr(e[f, 1], h * w // 4), Y.psnr(e[f, 2], h * w // 4))
            assert (res["psnr_y"][f], res["psnr_u"][f], res["psnr_v"][f]) == pytest.approx(p, rel=1e-12)
            assert res["psnr_yuv"][f] == pytest.approx((6 * p[0] + p[1] + p[2]) / 8, rel=1e-12)
