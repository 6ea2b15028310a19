"""CPU: the resampled render's sampling rule (render.View's tables), the CPU
statement of the forward against the native CPU render (bit for bit where the
rule is exact), decode_frames / decode_video with ``size`` and ``crop`` on a
CPU device, and the errors -- including the C entry's, which refuses bad
tables before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import resample_cases as RC
from gsvc_amd import codec
from gsvc_amd import compress as C
from gsvc_amd.render import View
from gsvc_amd.video import YuvFormat, rgb_to_i420


# --------------------------------------------------------------------------
# tables

def _check_axis(xd, p, starts, sample, src, out, start, extent):
    exd, ep, estarts = RC.axis(src, out, start, extent)
    assert np.array_equal(xd, exd) and np.array_equal(p, ep)
    assert np.array_equal(sample, exd.astype(np.float32))
    assert starts[0] == 0 and starts[-1] == out and len(starts) == (src + 15) // 16 + 1
    assert np.all(np.diff(starts) >= 0)
    assert np.array_equal(starts, estarts)
    # every column's owner tile is the one whose range holds it
    owner = np.searchsorted(starts, np.arange(out), side="right") - 1
    assert np.array_equal(owner, p >> 4)


def test_tables_sweep():
    """Source sizes 1..70 x output sizes 1..150: the whole frame, an integer
    window (columns) and a fractional one (rows)."""
    rng = np.random.default_rng(3)
    for s in range(1, 71):
        for o in range(1, 151):
            v = View(s, s, size=(o, o))
            _check_axis(v.xd, v.px, v.col_start, v.sample_x, s, o, 0.0, float(s))
            _check_axis(v.yd, v.py, v.row_start, v.sample_y, s, o, 0.0, float(s))
            w = int(rng.integers(1, s + 1))
            x0 = int(rng.integers(0, s - w + 1))
            h = float(rng.uniform(0.05, s))
            y0 = float(rng.uniform(0.0, s - h))
            v = View(s, s, size=(o, o), crop=(x0, y0, w, h))
            _check_axis(v.xd, v.px, v.col_start, v.sample_x, s, o, float(x0), float(w))
            _check_axis(v.yd, v.py, v.row_start, v.sample_y, s, o, y0, h)


def test_tables_exact_coordinates():
    """The three relations the bit-for-bit tests rest on."""
    for s in range(1, 71):
        v = View(s, 71 - s)
        assert v.is_identity
        assert np.array_equal(v.xd, np.arange(71 - s)) and np.array_equal(v.yd, np.arange(s))
        assert np.array_equal(v.px, np.arange(71 - s)) and np.array_equal(v.py, np.arange(s))
        for w in range(1, s + 1):
            for x0 in {0, (s - w) // 2, s - w}:
                v = View(s, s, size=(w, w), crop=(x0, x0, w, w))
                assert not v.is_identity or (x0 == 0 and w == s)
                assert np.array_equal(v.xd, x0 + np.arange(w)) and np.array_equal(v.yd, x0 + np.arange(w))
                for k in (3, 5, 7):
                    if k * w > 150:
                        continue
                    v = View(s, s, size=(k * w, k * w), crop=(x0, x0, w, w))
                    assert np.array_equal(v.xd[(k - 1) // 2::k], x0 + np.arange(w))
                    assert np.array_equal(v.px[(k - 1) // 2::k], x0 + np.arange(w))
                    assert np.array_equal(v.sample_y[(k - 1) // 2::k], (x0 + np.arange(w)).astype(np.float32))


def test_view_attributes():
    v = View(37, 53, size=(40, 90), crop=(10.25, 3.5, 20.5, 11.0))
    assert (v.out_h, v.out_w, v.src_h, v.src_w, v.is_identity) == (40, 90, 37, 53, False)
    sx, sy, cs, rs = v.host_tables()
    assert sx.dtype == np.float32 and sx.shape == (90,) and sy.shape == (40,)
    assert cs.dtype == np.int32 and cs.shape == (5,) and rs.shape == (4,)
    assert View(37, 53, size=(37, 53), crop=(0, 0, 53, 37)).is_identity
    assert not View(37, 53, size=(37, 53), crop=(0, 0, 52.5, 37)).is_identity


# --------------------------------------------------------------------------
# the CPU statement against the native CPU render

@pytest.fixture(scope="module")
def native():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = RC.native_cpu(RC.case(name))
        return cache[name]
    return get


@pytest.mark.parametrize("name", RC.CASES)
def test_identity_view_is_the_native_render(name, native):
    c = RC.case(name)
    out = RC.render(c, "cpu", View(c["H"], c["W"]))
    assert out.shape == native(name).shape and torch.equal(out, native(name))


@pytest.mark.parametrize("name", RC.CASES)
def test_integer_crop_is_the_native_window(name, native):
    c, crop = RC.case(name), RC.CROPS[name]
    out = RC.render(c, "cpu", View(c["H"], c["W"], size=(crop[3], crop[2]), crop=crop))
    assert torch.equal(out, RC.window(native(name), crop))


@pytest.mark.parametrize("name,k,cropped", RC.UPSCALES_CPU)
def test_odd_upscale_holds_the_native_samples(name, k, cropped, native):
    c = RC.case(name)
    crop = RC.CROPS[name] if cropped else (0, 0, c["W"], c["H"])
    out = RC.render(c, "cpu", View(c["H"], c["W"], size=(k * crop[3], k * crop[2]), crop=crop))
    assert out.shape[-2:] == (k * crop[3], k * crop[2])
    assert torch.equal(out[..., (k - 1) // 2::k, (k - 1) // 2::k], RC.window(native(name), crop))


def test_empty_frame_is_the_clamped_background(native):
    c = RC.case("batch")
    out = RC.render(c, "cpu", View(c["H"], c["W"], size=(30, 50), crop=(3.5, 2.25, 100, 60)))
    assert torch.equal(out[1], torch.tensor([0.25, 1.0, 0.0]).view(3, 1, 1).expand(3, 30, 50))
    assert float(out[0].std()) > 0


# --------------------------------------------------------------------------
# decode_frames / decode_video on a CPU device

def _unpacked(streams):
    """The decoded parameters of every frame, concatenated, and their sizes."""
    frames = C.unpack_frames_host(streams)
    T = torch.from_numpy
    xq = torch.cat([T(f[0]) for f in frames])
    Lq = torch.cat([T(f[1]) for f in frames])
    cq = torch.cat([T(f[2]) for f in frames])
    return xq, Lq, cq, [f[0].shape[0] for f in frames]


@pytest.mark.parametrize("kw", RC.STREAM_VIEWS)
def test_decode_frames_view_cpu(kw):
    from gsvc_amd.render import render_frames_sum
    streams = RC.stream()
    view = View(RC.STREAM_H, RC.STREAM_W, **kw)
    imgs, state = C.decode_frames(streams, "cpu", return_state=True, **kw)
    xq, Lq, cq, sizes = _unpacked(streams)
    want = render_frames_sum(xq, Lq, cq, sizes, RC.STREAM_H, RC.STREAM_W, torch.ones(3), view=view)
    assert imgs.shape == (3, 3, view.out_h, view.out_w) and torch.equal(imgs, want)
    _, state0 = C.decode_frames(streams, "cpu", return_state=True)
    assert all(torch.equal(a, b) for a, b in zip(state, state0))
    # two calls that carry prev
    a, st = C.decode_frames(streams[:1], "cpu", return_state=True, **kw)
    b = C.decode_frames(streams[1:], "cpu", prev=st, **kw)
    assert torch.equal(torch.cat([a, b]), imgs)


def test_decode_frames_identity_view_cpu():
    streams = RC.stream()
    assert torch.equal(C.decode_frames(streams, "cpu", size=(RC.STREAM_H, RC.STREAM_W)),
                       C.decode_frames(streams, "cpu"))


@pytest.mark.parametrize("fmt", [None, YuvFormat.from_pix_fmt("yuv420p10le"), YuvFormat.from_pix_fmt("nv12")])
def test_decode_frames_i420_view_cpu(fmt):
    streams = RC.stream()
    kw = dict(size=(90, 120), crop=(8, 4, 40, 30))
    imgs = C.decode_frames(streams, "cpu", **kw)
    yuv = C.decode_frames(streams, "cpu", output="i420", fmt=fmt, **kw)
    assert yuv.shape == (3, (fmt or YuvFormat()).frame_bytes(90, 120))
    assert torch.equal(yuv, rgb_to_i420(imgs, None, fmt))


def test_decode_video_size_cpu(tmp_path):
    streams = RC.stream()
    fmt = YuvFormat()
    outs = []
    for batch in (1, 8):
        path = tmp_path / f"b{batch}.yuv"
        res = codec.decode_video(streams, path, device="cpu", batch=batch, size=(24, 40))
        assert res["bytes_written"] == 3 * fmt.frame_bytes(24, 40) and res["frames"] == 3
        assert (res["height"], res["width"]) == (24, 40)
        outs.append(path.read_bytes())
    assert outs[0] == outs[1] and len(outs[0]) == 3 * fmt.frame_bytes(24, 40)
    want = C.decode_frames(streams, "cpu", output="i420", size=(24, 40))
    assert outs[0] == want.numpy().tobytes()
    res = codec.decode_video(streams, None, device="cpu")
    assert (res["height"], res["width"]) == (RC.STREAM_H, RC.STREAM_W)


def test_command_line_size_and_crop(tmp_path):
    streams = RC.stream()
    src, out = tmp_path / "a.gsvf", tmp_path / "a.yuv"
    codec.write_video(src, streams)
    res = codec.main(["decode", str(src), str(out), "--device", "cpu", "--size", "120x90",
                      "--crop", "8,4,40,30"])
    assert (res["height"], res["width"]) == (90, 120)
    want = C.decode_frames(streams, "cpu", output="i420", size=(90, 120), crop=(8, 4, 40, 30))
    assert out.read_bytes() == want.numpy().tobytes()


# --------------------------------------------------------------------------
# errors

@pytest.mark.parametrize("crop", [(-1, 0, 10, 10), (0, -0.5, 10, 10), (50, 0, 4, 10), (0, 30, 10, 8),
                                  (0, 0, 0, 10), (0, 0, 10, -1), (0, 0, 53.5, 37), (float("nan"), 0, 1, 1),
                                  (0, 0, 10)])
def test_crop_outside_the_frame(crop):
    with pytest.raises(ValueError):
        View(37, 53, crop=crop)
    with pytest.raises(ValueError):
        C.decode_frames(RC.stream(), "cpu", crop=(0, 0, RC.STREAM_W + 1, 4))


@pytest.mark.parametrize("size", [(0, 10), (10, 0), (-4, 8), (10,), (2.5, 4)])
def test_non_positive_size(size):
    with pytest.raises(ValueError):
        View(37, 53, size=size)
    with pytest.raises(ValueError):
        C.decode_frames(RC.stream(), "cpu", size=(0, 16))


def test_odd_size_for_420_and_reference():
    streams = RC.stream()
    for size in ((25, 40), (24, 41)):
        with pytest.raises(ValueError):
            C.decode_frames(streams, "cpu", output="i420", size=size)
        with pytest.raises(ValueError):
            codec.decode_video(streams, None, device="cpu", size=size)
    C.decode_frames(streams[:1], "cpu", output="yuv", fmt=YuvFormat.from_pix_fmt("yuv444p"), size=(25, 41))
    with pytest.raises(ValueError):  # 4:2:2: W even
        C.decode_frames(streams, "cpu", output="yuv", fmt=YuvFormat.from_pix_fmt("yuv422p"), size=(25, 41))
    ref = torch.zeros((3, YuvFormat().frame_bytes(24, 40)), dtype=torch.uint8)
    with pytest.raises(ValueError, match="reference"):
        C.decode_frames(streams, "cpu", output="i420", reference=ref, size=(24, 40))
    # the identity view may take one
    ref = torch.zeros((3, YuvFormat().frame_bytes(RC.STREAM_H, RC.STREAM_W)), dtype=torch.uint8)
    a = C.decode_frames(streams, "cpu", output="i420", reference=ref, size=(RC.STREAM_H, RC.STREAM_W))
    b = C.decode_frames(streams, "cpu", output="i420", reference=ref)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_view_of_another_frame_size():
    c = RC.case("edge")
    with pytest.raises(ValueError):
        RC.render(c, "cpu", View(c["H"] + 1, c["W"]))


def test_entry_refuses_bad_arguments_before_any_launch():
    """gsvc_render_frames_resampled returns GSVC_ERR_ARG from its host checks:
    no device is touched (this runs without one; the device pointers are never
    dereferenced)."""
    from gsvc_amd import _lib
    lib = _lib.load_product()
    H, W = 37, 53
    v = View(H, W, size=(40, 90))
    sx, sy, cs, rs = (a.copy() for a in v.host_tables())
    offs = (ctypes.c_int * 2)(0, 5)
    fake = 0x1000  # stands for a device buffer

    def call(**kw):
        a = dict(frames=1, offs=offs, offs_dev=fake, xyz=fake, chol=fake, feat=fake, bg=fake, H=H, W=W,
                 meta=fake, ws=fake, ws_bytes=1 << 30, sx=sx, sy=sy, cs=cs, rs=rs, sxd=fake, syd=fake,
                 csd=fake, rsd=fake, out_h=40, out_w=90, out=fake)
        a.update(kw)
        host = lambda t: t if t is None or isinstance(t, int) else t.ctypes.data
        rc = lib.gsvc_render_frames_resampled(
            a["frames"], a["offs"], a["offs_dev"], a["xyz"], 0, a["chol"], None, a["feat"], None, None,
            a["bg"], a["H"], a["W"], 0, 0, a["meta"], a["ws"], a["ws_bytes"], host(a["sx"]), host(a["sy"]),
            host(a["cs"]), host(a["rs"]), a["sxd"], a["syd"], a["csd"], a["rsd"], a["out_h"], a["out_w"],
            a["out"], None)
        return rc, lib.gsvc_last_error()

    def bad(t, i, val):
        t = t.copy()
        t[i] = val
        return t

    cases = [dict(cs=bad(cs, 0, 1)), dict(cs=bad(cs, -1, 89)), dict(cs=bad(cs, 2, cs[1] - 1)),
             dict(rs=bad(rs, 0, -1)), dict(rs=bad(rs, -1, 41)), dict(rs=bad(rs, 1, rs[2] + 1)),
             dict(out_w=91), dict(out_h=39)]
    for kw in cases:
        rc, msg = call(**kw)
        assert rc == 1 and b"partition" in msg, (kw, rc, msg)
    for key in ("offs_dev", "bg", "meta", "ws", "out", "sx", "sy", "cs", "rs", "sxd", "syd", "csd", "rsd",
                "xyz", "chol", "feat"):
        rc, msg = call(**{key: None})
        assert rc == 1 and b"missing" in msg, (key, rc, msg)
    for kw in (dict(out_h=0), dict(out_w=0), dict(frames=0), dict(H=0)):
        rc, msg = call(**kw)
        assert rc == 1 and b"bad sizes" in msg, (kw, rc, msg)
    rc, msg = call(sx=bad(sx, 3, np.float32("nan")))
    assert rc == 1 and b"sample_x" in msg
    rc, msg = call(sy=bad(sy, 0, np.float32(1e9)))
    assert rc == 1 and b"sample_y" in msg
