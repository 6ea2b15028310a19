"""CPU: the I420 output's arithmetic (premises, known answers, the round trip
through i420_to_rgb), the torch dispatch of ``rgb_to_i420`` against the numpy
statement (tests/yuv_cases.py), the C entry's argument errors, the container
(round trip and every validation rule on a hand-corrupted copy), the CPU
``decode_video`` and the command line."""
import ctypes
import json
import struct

import numpy as np
import pytest
import torch

import yuv_cases as Y

from gsvc_amd import codec
from gsvc_amd import compress as C
from gsvc_amd.video import rgb_to_i420

H, W = 32, 48
SIZE = H * W * 3 // 2
GOP = [(65, True), (50, False), (33, False), (71, True), (41, False)]  # (splats, key frame)


# --------------------------------------------------------------------------
# premises

def test_quantizer_inverts_the_255_grid():
    k = np.arange(256)
    assert np.array_equal(Y.quantize(k.astype(np.float32) / np.float32(255)), k)
    x = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 2.0, -1.0], np.float32)
    assert Y.quantize(x).tolist() == [0, 255, 0, 0, 0, 255, 255, 0]


def test_accumulators_fit_int32_and_are_not_negative():
    lo_hi = []
    for coef, bias, top in (((269484, 528482, 102760), (16 << 20) + (1 << 19), 255),
                            ((-155188, -305135, 460324), (128 << 22) + (1 << 21), 1020),
                            ((460324, -385875, -74448), (128 << 22) + (1 << 21), 1020)):
        lo_hi.append((bias + top * sum(c for c in coef if c < 0), bias + top * sum(c for c in coef if c > 0)))
    assert min(lo for lo, _ in lo_hi) >= 0
    assert max(hi for _, hi in lo_hi) == 1008498544 < 2 ** 31


@pytest.mark.parametrize("rgb, yuv", [((0, 0, 0), (16, 128, 128)), ((1, 1, 1), (235, 128, 128)),
                                      ((1, 0, 0), (82, 90, 240)), ((0, 1, 0), (145, 54, 34)),
                                      ((0, 0, 1), (41, 240, 110))])
def test_known_answers_for_flat_blocks(rgb, yuv):
    img = np.broadcast_to(np.array(rgb, np.float32).reshape(1, 3, 1, 1), (1, 3, 2, 2))
    assert Y.rgb_to_i420(img)[0].tolist() == [yuv[0]] * 4 + [yuv[1], yuv[2]]
    assert rgb_to_i420(torch.from_numpy(img.copy()))[0].tolist() == [yuv[0]] * 4 + [yuv[1], yuv[2]]


def test_round_trip_through_i420_to_rgb(oracle):
    """Flat 2x2 blocks over ALL legal (Y 16..235, U, V 16..240) whose
    oracle.i420_to_rgb image is unclipped (every channel's 20-bit value inside
    [0, 255] before the saturation): forward o inverse gives |dY| <= 1 and U, V
    exact; unclipped share 23.6 %, max errors 1 / 0 / 0."""
    u, v = (a.ravel() for a in np.meshgrid(np.arange(16, 241), np.arange(16, 241), indexing="ij"))
    n = u.size
    kept = total = 0
    worst = [0, 0, 0]
    for y in range(16, 236):
        # yuv.hip's constants, before its clamp: which blocks the inverse does not clip
        yy = max(0, y - 16) * 1220542 + (1 << 19)
        r = (yy + 1673527 * (v - 128)) >> 20
        g = (yy - 852492 * (v - 128) - 409993 * (u - 128)) >> 20
        b = (yy + 2116026 * (u - 128)) >> 20
        ok = np.ones(n, bool)
        for ch in (r, g, b):
            ok &= (ch >= 0) & (ch <= 255)
        total += n
        kept += int(ok.sum())
        if not ok.any():
            continue
        frame = np.concatenate([np.full(4 * n, y, np.uint8), u.astype(np.uint8), v.astype(np.uint8)])
        rgb = oracle.i420_to_rgb(frame, 2, 2 * n)  # [3, 2, 2n]: block k at columns 2k, 2k+1
        q = Y.quantize(rgb[:, 0, ::2])
        assert np.array_equal(Y.quantize(rgb), np.repeat(np.repeat(q[:, None, :], 2, 1), 2, 2))  # flat
        y2 = Y.luma(q[0], q[1], q[2])
        u2, v2 = Y.chroma(4 * q[0], 4 * q[1], 4 * q[2])
        for k, (got, want) in enumerate(((y2, y), (u2, u), (v2, v))):
            worst[k] = max(worst[k], int(np.abs(got - want)[ok].max()))
    share = kept / total
    print(f"unclipped share {share:.4f}, max errors {worst}")
    assert abs(share - 0.236) < 0.0005
    assert worst == [1, 0, 0]


# --------------------------------------------------------------------------
# the torch dispatch against the numpy statement

@pytest.mark.parametrize("kind", Y.CLASSES)
@pytest.mark.parametrize("shape", Y.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_torch_dispatch_equals_numpy(shape, kind):
    h, w = shape
    for f in Y.FRAMES:
        x = Y.values(kind, f, h, w)
        want = Y.rgb_to_i420(x)
        got = rgb_to_i420(torch.from_numpy(x))
        assert got.dtype == torch.uint8 and got.shape == (f, h * w * 3 // 2)
        assert np.array_equal(got.numpy(), want)
        ref = Y.reference_frames(f, h, w)
        got2, sse = rgb_to_i420(torch.from_numpy(x), torch.from_numpy(ref))
        assert np.array_equal(got2.numpy(), want)
        assert sse.dtype == torch.int64 and np.array_equal(sse.numpy(), Y.sse(want, ref, h, w))
        _, zero = rgb_to_i420(torch.from_numpy(x), torch.from_numpy(want))
        assert not zero.any()


def test_torch_dispatch_input_forms():
    x = Y.values("uniform", 2, 6, 10)
    want = Y.rgb_to_i420(x)
    t = torch.from_numpy(x)
    assert np.array_equal(rgb_to_i420(t[0]).numpy(), want[:1])  # [3, H, W]
    hwc = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)  # not contiguous
    assert not hwc.is_contiguous() and np.array_equal(rgb_to_i420(hwc).numpy(), want)
    assert np.array_equal(rgb_to_i420(t.double()).numpy(), want)  # float32 first
    for bad in (t[:, :2], t[:, :, :5], t.to(torch.int32)):
        with pytest.raises(ValueError):
            rgb_to_i420(bad)
    with pytest.raises(ValueError):
        rgb_to_i420(t, torch.zeros(3, dtype=torch.uint8))


def test_c_entry_argument_errors_without_launch():
    from gsvc_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)  # never dereferenced: the argument checks fail first
    cases = [((0, p, 2, 2, p, None, None), b"frames"), ((-1, p, 2, 2, p, None, None), b"frames"),
             ((1, p, 0, 2, p, None, None), b"even"), ((1, p, 2, -2, p, None, None), b"even"),
             ((1, p, 3, 2, p, None, None), b"even"), ((1, p, 2, 6 + 1, p, None, None), b"even"),
             ((1, None, 2, 2, p, None, None), b"missing buffer"),
             ((1, p, 2, 2, None, None, None), b"missing buffer"),
             ((1, p, 2, 2, p, p, None), b"sse")]
    for args, msg in cases:
        assert lib.gsvc_rgb_to_i420(*args, None) == 1, args
        assert msg in lib.gsvc_last_error(), (args, lib.gsvc_last_error())


# --------------------------------------------------------------------------
# the container

def _gop_cpu(plan=GOP, h=H, w=W, seed=5):
    """Frame streams of untrained models on the CPU (as test_quantize_gpu's
    _gop): every delta model holds the decoded parameters of the frame before
    it; versions 1 and 2 alternate."""
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
    imgs = C.decode_frames(streams, "cpu")
    return streams, Y.rgb_to_i420(imgs.numpy())


def _assemble(streams, h=H, w=W, fps=(30, 1)):
    """The container's bytes, from the format's table alone."""
    offs, o = [], 64
    for s in streams:
        offs.append(o)
        o += len(s)
    head = struct.pack("<4sIIIIIIIQQ", b"GSVF", 1, h, w, len(streams), fps[0], fps[1], 0, o,
                       o + 16 * len(streams))
    index = b"".join(struct.pack("<QII", off, len(s), struct.unpack_from("<I", s, 20)[0] & 1)
                     for off, s in zip(offs, streams))
    return head + bytes(64 - len(head)) + b"".join(streams) + index


def test_container_round_trip(gop, tmp_path):
    streams, _ = gop
    path = tmp_path / "a.gsvf"
    size = codec.write_video(path, streams, fps=(30000, 1001))
    blob = path.read_bytes()
    assert size == len(blob) and blob == _assemble(streams, fps=(30000, 1001))
    vid = codec.read_video(path)
    assert (vid.H, vid.W, vid.num_frames, vid.fps) == (H, W, 5, (30000, 1001))
    assert vid.key_frames == [0, 3] and vid.sizes == [n for n, _ in GOP]
    assert vid.versions == [1, 2, 1, 2, 1]
    assert [vid.frame(i) for i in range(5)] == list(streams)
    assert [list(vid.span(i)) for i in range(5)] == [[0], [0, 1], [0, 1, 2], [3], [3, 4]]
    with pytest.raises(IndexError):
        vid.frame(5)
    with pytest.raises(ValueError):
        codec.write_video(tmp_path / "b.gsvf", [])
    with pytest.raises(ValueError, match="delta"):
        codec.write_video(tmp_path / "b.gsvf", streams[1:])


def _patch(blob, offset, fmt, *values):
    b = bytearray(blob)
    struct.pack_into(fmt, b, offset, *values)
    return bytes(b)


def test_container_validation(gop, tmp_path):
    """Every rule of read_video on a hand-corrupted copy: ValueError before
    anything is decoded."""
    streams, _ = gop
    good = _assemble(streams)
    n = len(streams)
    io = struct.unpack_from("<Q", good, 32)[0]  # index_offset
    entry = [struct.unpack_from("<QII", good, io + 16 * i) for i in range(n)]
    swapped = bytearray(good)
    swapped[io:io + 16], swapped[io + 16:io + 32] = good[io + 16:io + 32], good[io:io + 16]
    short = _assemble([streams[0], streams[1]])  # frame 0's entry cut by one splat, a gap after it
    short_io = struct.unpack_from("<Q", short, 32)[0]
    first_delta = _patch(_patch(good, 64 + 20, "<I", 1), io + 12, "<I", 1)
    bad = {
        "magic": (_patch(good, 0, "<4s", b"GSVQ"), "magic"),
        "version": (_patch(good, 4, "<I", 2), "version"),
        "real size": (good + b"\0", "file_bytes"),
        "truncated": (good[:-1], "file_bytes"),
        "index size": (_patch(good, 32, "<Q", io - 16), "file_bytes"),
        "frames": (_patch(good, 16, "<I", n + 1), "file_bytes"),
        "ascending": (bytes(swapped), "ascend"),
        "overlap": (_patch(good, io + 16, "<Q", entry[1][0] - 1), "overlap"),
        "in header": (_patch(good, io, "<Q", 48), "ascend"),
        "past the streams": (_patch(good, io + 16 * (n - 1) + 8, "<I", entry[-1][1] + 16), "inside"),
        "too short": (_patch(good, io + 8, "<I", 100), "inside"),
        "own length": (_patch(short, short_io + 8, "<I", len(streams[0]) - 7), "frame 0"),
        "own length v2": (_patch(short, short_io + 16, "<QI", entry[1][0] + 2, entry[1][1] - 2), "frame 1"),
        "frame size": (_patch(good, 8, "<I", H + 16), "the video"),
        "frame width": (_patch(good, 12, "<I", W - 16), "the video"),
        "first delta": (first_delta, "frame 0 is a delta"),
        "delta grows": (_assemble([streams[0], streams[2], streams[1]]), "predecessor"),
        "index flag": (_patch(good, io + 12, "<I", 1), "delta flag"),
        "short file": (good[:40], "shorter"),
    }
    path = tmp_path / "bad.gsvf"
    for name, (blob, msg) in bad.items():
        path.write_bytes(blob)
        with pytest.raises(ValueError, match=msg):
            codec.read_video(path)
        with pytest.raises(ValueError, match=msg):  # the decoder refuses it before it decodes
            codec.decode_video(str(path), device="cpu")
    path.write_bytes(good)
    assert codec.read_video(path).num_frames == n


# --------------------------------------------------------------------------
# the CPU decoder

def test_decode_video_cpu(gop, tmp_path):
    streams, want = gop
    path, out = tmp_path / "a.gsvf", tmp_path / "a.yuv"
    codec.write_video(path, streams)
    src = Y.reference_frames(5, H, W, seed=3)
    (tmp_path / "src.yuv").write_bytes(src.tobytes())
    r8 = codec.decode_video(str(path), str(out), device="cpu", batch=8, reference=str(tmp_path / "src.yuv"))
    assert r8["frames"] == 5 and r8["bytes_written"] == 5 * SIZE and r8["seconds"] > 0
    assert out.read_bytes() == want.tobytes()
    r2 = codec.decode_video(str(path), str(tmp_path / "b.yuv"), device="cpu", batch=2,
                            reference=str(tmp_path / "src.yuv"))
    assert (tmp_path / "b.yuv").read_bytes() == want.tobytes()
    r1 = codec.decode_video(list(streams), str(tmp_path / "c.yuv"), device="cpu", batch=1)  # a stream list
    assert (tmp_path / "c.yuv").read_bytes() == want.tobytes() and "psnr_y" not in r1
    # a range starts at its GOP's key frame and drops what precedes it
    r = codec.decode_video(str(path), str(tmp_path / "d.yuv"), device="cpu", batch=2, frames=range(3, 5))
    assert r["frames"] == 2 and (tmp_path / "d.yuv").read_bytes() == want[3:5].tobytes()
    codec.decode_video(str(path), str(tmp_path / "e.yuv"), device="cpu", batch=8, frames=range(2, 4))
    assert (tmp_path / "e.yuv").read_bytes() == want[2:4].tobytes()
    for bad in (range(0, 6), range(3, 3), range(0, 4, 2)):
        with pytest.raises(ValueError):
            codec.decode_video(str(path), device="cpu", frames=bad)
    # PSNR in the 8-bit domain, from the bytes
    e = Y.sse(want, src, H, W)
    for res in (r8, r2):
        for f in range(5):
            py, pu, pv = (Y.psnr(e[f, 0], H * W), Y.psnr(e[f, 1], H * W // 4), Y.psnr(e[f, 2], H * W // 4))
            assert (res["psnr_y"][f], res["psnr_u"][f], res["psnr_v"][f]) == pytest.approx((py, pu, pv), rel=1e-12)
            assert res["psnr_yuv"][f] == pytest.approx((6 * py + pu + pv) / 8, rel=1e-12)
    (tmp_path / "same.yuv").write_bytes(want.tobytes())
    same = codec.decode_video(str(path), device="cpu", reference=str(tmp_path / "same.yuv"))
    assert same["bytes_written"] == 0
    assert all(np.isinf(p) for k in ("psnr_y", "psnr_u", "psnr_v", "psnr_yuv") for p in same[k])


def test_decode_frames_i420_cpu(gop):
    streams, want = gop
    imgs, st = C.decode_frames(streams[:3], "cpu", return_state=True)
    out, st2 = C.decode_frames(streams[:3], "cpu", return_state=True, output="i420")
    assert imgs.dtype == torch.float32 and np.array_equal(out.numpy(), want[:3])
    assert all(torch.equal(a, b) for a, b in zip(st, st2))
    tail = C.decode_frames(streams[1:3], "cpu", prev=C.decode_frames(streams[:1], "cpu", return_state=True)[1],
                           output="i420")
    assert np.array_equal(tail.numpy(), want[1:3])
    with pytest.raises(ValueError):
        C.decode_frames(streams, "cpu", output="yuv")


# --------------------------------------------------------------------------
# the command line

def test_adan_step_cpu_dispatch_follows_the_foreach_sequence():
    """The encoder's optimizer on a host without a GPU: ops.adan_step on CPU
    tensors against the reference's foreach sequence (tools/foreach_adan.py),
    three steps, both proximal forms; float32 rounding of the scalars aside."""
    from foreach_adan import foreach_adan
    from gsvc_amd import ops
    g = torch.Generator().manual_seed(2)
    for no_prox in (False, True):
        a = [[torch.randn(37, 3, generator=g)] for _ in range(6)]
        a[3][0].abs_()  # exp_avg_sq
        b = [[t[0].clone()] for t in a]
        for t in range(1, 4):
            kw = dict(beta1=0.98, beta2=0.92, beta3=0.99, bias_correction1=1 - 0.98 ** t,
                      bias_correction2=1 - 0.92 ** t, bias_correction3_sqrt=(1 - 0.99 ** t) ** 0.5, lr=1e-2,
                      weight_decay=0.1, eps=1e-8, no_prox=no_prox, clip_global_grad_norm=1.0)
            grad = torch.randn(37, 3, generator=g)
            a[1][0], b[1][0] = grad.clone(), grad.clone()
            ops.adan_step(*a, **kw)
            foreach_adan(*b, **kw)
            assert torch.equal(a[1][0], grad)  # gradients are read only
            for x, y in zip(a, b):
                torch.testing.assert_close(x[0], y[0], rtol=1e-5, atol=1e-6)


def test_cli_encode_info_decode(tmp_path, capsys):
    h = w = 32
    frames, n = 3, 40
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    src = bytearray()
    for f in range(frames):
        src += ((xx * 5 + yy * 3 + 20 * f) % 220 + 16).astype(np.uint8).tobytes()
        src += np.full(h * w // 4, 100 + 10 * f, np.uint8).tobytes() + np.full(h * w // 4, 140, np.uint8).tobytes()
    (tmp_path / "src.yuv").write_bytes(bytes(src))
    g = torch.Generator().manual_seed(11)
    models = {f"frame_{f + 1}": {"_xyz": torch.atanh(1.8 * (torch.rand(n, 2, generator=g) - 0.5)),
                                 "_cholesky": 3.0 * torch.rand(n, 3, generator=g),
                                 "_features_dc": torch.rand(n, 3, generator=g)} for f in range(frames)}
    torch.save(models, tmp_path / "models.pth")
    enc = codec.main(["encode", str(tmp_path / "models.pth"), str(tmp_path / "src.yuv"),
                      str(tmp_path / "v.gsvf"), "--width", str(w), "--height", str(h), "--iterations", "2",
                      "--k_frames", "1,3", "--entropy", "--seed", "3", "--device", "cpu"])
    assert enc["frames"] == frames and enc["file_bytes"] == (tmp_path / "v.gsvf").stat().st_size
    capsys.readouterr()
    info = codec.main(["info", str(tmp_path / "v.gsvf")])
    printed = json.loads(capsys.readouterr().out)
    assert printed == info
    assert (info["H"], info["W"], info["frames"], info["key_frames"]) == (h, w, frames, [0, 2])
    dec = codec.main(["decode", str(tmp_path / "v.gsvf"), str(tmp_path / "out.yuv"), "--device", "cpu",
                      "--batch", "2", "--reference", str(tmp_path / "src.yuv")])
    assert (tmp_path / "out.yuv").stat().st_size == frames * h * w * 3 // 2 == dec["bytes_written"]
    assert len(dec["psnr_yuv"]) == frames
    part = codec.main(["decode", str(tmp_path / "v.gsvf"), str(tmp_path / "part.yuv"), "--device", "cpu",
                       "--frames", "1:3"])
    assert part["frames"] == 2
    assert (tmp_path / "part.yuv").read_bytes() == (tmp_path / "out.yuv").read_bytes()[h * w * 3 // 2:]
