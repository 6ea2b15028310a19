"""GPU: the resampled composite (csrc/resample.hip) against the native batched
render, bit for bit where the sampling rule is exact -- the identity view,
integer windows at scale 1, the native samples inside odd upscales --, against
the CPU statement elsewhere, and through decode_frames / decode_video."""
import numpy as np
import pytest
import torch

import resample_cases as RC
from gsvc_amd import codec
from gsvc_amd import compress as C
from gsvc_amd.render import View, render_frames_sum
from gsvc_amd.video import YuvFormat, rgb_to_i420

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native(cuda):
    """The native batched render of each case, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = RC.render(RC.case(name), cuda)
        return cache[name]
    return get


@pytest.mark.parametrize("name", RC.CASES)
def test_identity_view_is_the_native_render(cuda, name, native):
    c = RC.case(name)
    want = native(name)
    out = RC.render(c, cuda, View(c["H"], c["W"]))
    assert out.shape == want.shape and torch.equal(out, want)
    # the two entries alternate on one workspace
    assert torch.equal(RC.render(c, cuda), want)
    assert torch.equal(RC.render(c, cuda, View(c["H"], c["W"])), want)


@pytest.mark.parametrize("name", RC.CASES)
def test_integer_crop_is_the_native_window(cuda, name, native):
    c, crop = RC.case(name), RC.CROPS[name]
    out = RC.render(c, cuda, View(c["H"], c["W"], size=(crop[3], crop[2]), crop=crop))
    assert torch.equal(out, RC.window(native(name), crop))


@pytest.mark.parametrize("name,k,cropped", RC.UPSCALES)
def test_odd_upscale_holds_the_native_samples(cuda, name, k, cropped, native):
    c = RC.case(name)
    crop = RC.CROPS[name] if cropped else (0, 0, c["W"], c["H"])
    out = RC.render(c, cuda, View(c["H"], c["W"], size=(k * crop[3], k * crop[2]), crop=crop))
    assert out.shape[-2:] == (k * crop[3], k * crop[2])
    assert torch.equal(out[..., (k - 1) // 2::k, (k - 1) // 2::k], RC.window(native(name), crop))


def _views(c):
    H, W = c["H"], c["W"]
    return [dict(size=(2 * H, 2 * W)), dict(size=(H // 2, W // 2)), dict(size=(40, 90)),
            dict(crop=(10.25, 3.5, 20.5, 11.0))]


@pytest.mark.parametrize("name", RC.CASES)
@pytest.mark.parametrize("which", range(4))
def test_against_the_cpu_statement(cuda, name, which):
    """2x, 0.5x, a non-uniform size and a fractional window (a zoom): no exact
    relation, so the CPU statement's image at the forward tests' image bar."""
    c = RC.case(name)
    view = View(c["H"], c["W"], **_views(c)[which])
    got = RC.render(c, cuda, view).cpu().numpy()
    want = RC.render(c, "cpu", view).numpy()
    err = float(np.max(np.abs(got - want)))
    print(f"{name} view {which}: {got.shape}, max |gpu - cpu| = {err:.3e}")
    np.testing.assert_allclose(got, want, rtol=RC.IMG_RTOL, atol=RC.IMG_ATOL)


def test_empty_rectangles_and_background(cuda):
    """A strong downscale and a small window: most source tiles own no sample;
    the all-degenerate frame is the clamped background at every size."""
    c = RC.case("batch")
    for kw in (dict(size=(3, 5)), dict(size=(1, 1)), dict(size=(9, 7), crop=(100.5, 60.25, 3.0, 2.5))):
        view = View(c["H"], c["W"], **kw)
        out = RC.render(c, cuda, view)
        bgimg = torch.tensor([0.25, 1.0, 0.0], device=cuda).view(3, 1, 1).expand(3, view.out_h, view.out_w)
        assert torch.equal(out[1], bgimg)
        np.testing.assert_allclose(out.cpu().numpy(), RC.render(c, "cpu", view).numpy(),
                                   rtol=RC.IMG_RTOL, atol=RC.IMG_ATOL)


# --------------------------------------------------------------------------
# decode_frames / decode_video

@pytest.mark.parametrize("kw", RC.STREAM_VIEWS)
def test_decode_frames_view(cuda, kw):
    streams = RC.stream()
    view = View(RC.STREAM_H, RC.STREAM_W, **kw)
    imgs, state = C.decode_frames(streams, cuda, return_state=True, **kw)
    xq, Lq, cq, _, sizes, (H, W) = C.unpack_frames(streams, cuda)
    want = render_frames_sum(xq, Lq, cq, sizes, H, W, torch.ones(3, device=cuda), view=view)
    assert imgs.shape == (3, 3, view.out_h, view.out_w) and torch.equal(imgs, want)
    _, state0 = C.decode_frames(streams, cuda, return_state=True)
    assert all(torch.equal(a, b) for a, b in zip(state, state0))
    # two calls that carry prev
    a, st = C.decode_frames(streams[:1], cuda, return_state=True, **kw)
    b = C.decode_frames(streams[1:], cuda, prev=st, **kw)
    assert torch.equal(torch.cat([a, b]), imgs)


def test_decode_frames_identity_and_windows(cuda):
    streams = RC.stream()
    native = C.decode_frames(streams, cuda)
    assert torch.equal(C.decode_frames(streams, cuda, size=(RC.STREAM_H, RC.STREAM_W)), native)
    assert torch.equal(C.decode_frames(streams, cuda, crop=(8, 4, 40, 30), size=(30, 40)),
                       native[..., 4:34, 8:48])
    up = C.decode_frames(streams, cuda, crop=(8, 4, 40, 30), size=(90, 120))
    assert torch.equal(up[..., 1::3, 1::3], native[..., 4:34, 8:48])


@pytest.mark.parametrize("fmt", [None, YuvFormat.from_pix_fmt("yuv420p10le"), YuvFormat.from_pix_fmt("nv12")])
def test_decode_frames_i420_view(cuda, fmt):
    streams = RC.stream()
    kw = dict(size=(90, 120), crop=(8, 4, 40, 30))
    imgs = C.decode_frames(streams, cuda, **kw)
    yuv = C.decode_frames(streams, cuda, output="i420", fmt=fmt, **kw)
    assert yuv.shape == (3, (fmt or YuvFormat()).frame_bytes(90, 120))
    assert torch.equal(yuv, rgb_to_i420(imgs, None, fmt))


def test_decode_video_size(cuda, tmp_path):
    streams = RC.stream()
    fmt = YuvFormat()
    outs = []
    for batch in (1, 8):
        path = tmp_path / f"b{batch}.yuv"
        res = codec.decode_video(streams, path, device=cuda, batch=batch, size=(96, 160))
        assert res["bytes_written"] == 3 * fmt.frame_bytes(96, 160) and res["frames"] == 3
        assert (res["height"], res["width"]) == (96, 160)
        outs.append(path.read_bytes())
    assert outs[0] == outs[1] and len(outs[0]) == 3 * fmt.frame_bytes(96, 160)
    want = C.decode_frames(streams, cuda, output="i420", size=(96, 160))
    assert outs[0] == want.cpu().numpy().tobytes()
