"""GPU: the device transcoding of the entropy-coded stream (csrc/ans.hip)
against the host decoder byte for byte, and the decode of coded and mixed
GOPs against the version-1 GOP bit for bit."""
import ctypes
import math

import numpy as np
import pytest
import torch

import entropy_cases as E
import quant_cases as Q
from gsvc_amd import _lib
from gsvc_amd import ans
from gsvc_amd import compress as C

pytestmark = pytest.mark.gpu

H, W = E.H, E.W
_coded = {}


def coded(n, S, delta=False):
    """(version-1 stream, its version-2 coding), computed once."""
    k = (n, S, delta)
    if k not in _coded:
        s = E.case_stream(n, delta)
        _coded[k] = (s, ans.entropy_code(s, S))
    return _coded[k]


def expand_on_device(streams):
    """gsvc_expand_stream on the concatenated list: the expanded bytes read
    back, and the offsets gsvc_stream_expanded_bytes gave.  The output buffer
    is 64 bytes longer than asked for and filled with 0xa5: nothing past the
    expanded stream may change."""
    lib = _lib.load()
    blob = b"".join(streams)
    offs = [0]
    for s in streams:
        offs.append(offs[-1] + len(s))
    arr = (ctypes.c_longlong * len(offs))(*offs)
    exp = (ctypes.c_longlong * len(offs))()
    assert lib.gsvc_stream_expanded_bytes(len(streams), ctypes.c_char_p(blob), arr, exp) == 0
    total = exp[len(streams)]
    dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    out = torch.full((total + 64,), 0xa5, dtype=torch.uint8, device="cuda")
    _lib.call("gsvc_expand_stream", len(streams), ctypes.c_char_p(blob), arr, _lib.ptr(dev),
              _lib.ptr(out), total, _lib.stream(out.device))
    got = out.cpu().numpy().tobytes()
    assert got[total:] == b"\xa5" * 64
    return got[:total], list(exp)


@pytest.mark.parametrize("S", E.SEGMENTS)
@pytest.mark.parametrize("n", E.SIZES)
def test_device_transcoding(cuda, n, S):
    for delta in (False, True):
        v1, v2 = coded(n, S, delta)
        got, offs = expand_on_device([v2])
        assert offs == [0, len(v1)]
        assert got == ans.entropy_expand(v2) == v1


def test_device_transcoding_edge_histograms(cuda):
    for s, S in ((E.constant_stream(300), 64), (E.rare_stream(), 64), (E.all_bytes_stream(), 128),
                 (E.delta_like_stream(), 32)):
        got, _ = expand_on_device([ans.entropy_code(s, S)])
        assert got == s


def test_device_transcoding_of_lists(cuda):
    """A version-2 frame at an odd byte offset (behind a version-1 frame of odd
    N), frames of different N and S in one call, F = 1 and F = 8, and more
    frames than one launch takes."""
    odd = coded(63, 64)[0]
    assert len(odd) % 2 == 1
    frames = [odd, coded(300, 64)[1], coded(65, 32, True)[1], coded(4099, 128)[1], coded(64, 1)[0],
              coded(1, 64, True)[1], coded(0, 64)[1], coded(300, 4096, True)[1]]
    want = b"".join(s if C.parse_header(s)["version"] == 1 else ans.entropy_expand(s) for s in frames)
    got, offs = expand_on_device(frames)
    assert len(frames) == 8 and got == want and offs[-1] == len(want)
    assert expand_on_device(frames[:2])[0] == want[:offs[2]]
    assert expand_on_device([frames[1]])[0] == want[offs[1]:offs[2]]
    many = [frames[k % 3] for k in range(35)]  # 35 > the 32 frames of one launch
    want = b"".join(s if C.parse_header(s)["version"] == 1 else ans.entropy_expand(s) for s in many)
    assert expand_on_device(many)[0] == want


def _same(a, b):
    assert a[4] == b[4] and a[5] == b[5]
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)


def test_decode_of_coded_and_mixed_gops(cuda):
    """A key frame and two deltas, the second with fewer splats: all coded, and
    mixed [v2, v1, v2], equal the version-1 list; so does a prev state carried
    across two calls; two runs give equal bits."""
    key = Q.make_case(300)
    ref0 = Q.ref_forward(key)
    d1 = dict(Q.make_case(300, seed=1, delta=True))
    d1["prev"] = (ref0["xq"], ref0["Lpre"], ref0["cq"])
    ref1 = Q.ref_forward(d1)
    d2 = dict(Q.make_case(65, seed=2, delta=True))
    d2["prev"] = tuple(ref1[k][:65] for k in ("xq", "Lpre", "cq"))
    v1 = [C.encode_frame(Q.model_from_case(c, H, W, device="cuda")) for c in (key, d1, d2)]
    v2 = [C.encode_frame(Q.model_from_case(c, H, W, device="cuda"), entropy=True, segment=S)
          for c, S in zip((key, d1, d2), (64, 32, 128))]
    assert [ans.entropy_expand(s) for s in v2] == v1
    want = C.unpack_frames(v1, "cuda")
    np.testing.assert_array_equal(want[0][300:600].cpu().numpy(), ref1["xq"])
    for streams in (v2, [v2[0], v1[1], v2[2]], [v1[0], v2[1], v1[2]]):
        _same(C.unpack_frames(streams, "cuda"), want)
    imgs = C.decode_frames(v1, "cuda")
    a = C.decode_frames(v2, "cuda")
    b = C.decode_frames([v2[0], v1[1], v2[2]], "cuda")
    assert torch.equal(a, imgs) and torch.equal(b, imgs) and float(imgs.std()) > 0
    assert torch.equal(C.decode_frames(v2, "cuda"), a)  # two runs
    # the state carried from a first call into a second
    first, state = C.decode_frames(v2[:1], "cuda", return_state=True)
    rest, last = C.decode_frames(v2[1:], "cuda", prev=state, return_state=True)
    assert torch.equal(torch.cat([first, rest]), imgs)
    _, last1 = C.decode_frames(v1, "cuda", return_state=True)
    assert all(torch.equal(x, y) for x, y in zip(last, last1))


def test_coded_gop_equals_the_trained_renders(cuda):
    """A GOP built as test_quantize_gpu.test_gop_decode_bit_equal builds its
    own: each delta on the decoded parameters of the frame before, so the
    decoded images are the models' eval renders."""
    torch.manual_seed(5)
    kw = dict(H=H, W=W, BLOCK_H=16, BLOCK_W=16, device="cuda", lr=1e-3, quantize=True, opt_type="adan")
    models, streams, state = [], [], None
    for n in (257, 200, 65):
        if state is None:
            m = C.GaussianVideoFrameQ(num_points=n, **kw).cuda()
            with torch.no_grad():
                m._cholesky.mul_(3.0)
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
        s = C.encode_frame(m, entropy=True)
        assert C.parse_header(s)["version"] == 2 and ans.entropy_expand(s) == C.encode_frame(m)
        xq, _, cq, Lpre, _, _ = C.unpack_frames([s], "cuda", prev=state)
        state = (xq, Lpre, cq)
        models.append(m)
        streams.append(s)
    imgs = C.decode_frames(streams, "cuda")
    assert imgs.shape == (3, 3, H, W)
    for f, m in enumerate(models):
        with torch.no_grad():
            assert torch.equal(imgs[f], m.forward_quantize()["render"][0]), f


def test_compress_video_entropy(cuda):
    from gsvc_amd.frame import synthetic_gt
    torch.manual_seed(3)
    frames = [synthetic_gt(H, W, s, "cuda") for s in (1, 2, 3)]
    sd = {}
    for i, n in enumerate((65, 65, 40)):
        sd[f"frame_{i + 1}"] = {"_xyz": torch.atanh(2 * (torch.rand(n, 2) - 0.5)).cuda(),
                                "_cholesky": (3 * torch.rand(n, 3)).cuda(),
                                "_features_dc": torch.rand(n, 3).cuda()}
    out = C.compress_video(sd, frames, K_frames=[1], iterations=3, lr=1e-2, device="cuda",
                           delta_base="decoded", seed=0, entropy=True, segment=32)
    heads = [C.parse_header(s) for s in out["streams"]]
    assert [h["version"] for h in heads] == [2, 2, 2] and [h["S"] for h in heads] == [32, 32, 32]
    assert [h["N"] for h in heads] == [65, 65, 40]
    assert [h["delta"] for h in heads] == [False, True, True]
    assert out["bpp_coded"] == [8 * len(s) / H / W for s in out["streams"]]
    assert out["bpp"] == [8 * (256 + 7 * n) / H / W for n in (65, 65, 40)]
    imgs = C.decode_frames(out["streams"], "cuda")
    for f in range(3):  # the decoded GOP reproduces the PSNR the loop measured on its eval renders
        mse = torch.nn.functional.mse_loss(imgs[f:f + 1], frames[f]).item()
        assert 10 * math.log10(1.0 / mse) == out["psnr"][f], f
    plain = C.compress_video(sd, frames[:1], K_frames=[1], iterations=1, lr=1e-2, device="cuda", seed=0)
    assert set(plain) == {"streams", "psnr", "bpp", "bpp_entropy_estimate", "state_dicts"}
    assert len(plain["streams"][0]) == 256 + 7 * 65


def test_unpack_stream_launches_nothing_on_errors(cuda):
    """A workspace one byte short, and a corrupt host copy: status 2 / 1 and the
    outputs keep their fill."""
    lib = _lib.load()
    v1, v2 = coded(65, 32)
    out = torch.full((65 * 8,), 7.0, device="cuda")
    work = torch.full((len(v1),), 0xa5, dtype=torch.uint8, device="cuda")
    bound = torch.tensor([0.5, 0.0, 0.5], device="cuda")
    dev = torch.frombuffer(bytearray(v2), dtype=torch.uint8).cuda()
    p = ctypes.c_void_p(out.data_ptr())

    def call(buf, workspace_bytes):
        arr = (ctypes.c_longlong * 2)(0, len(buf))
        rc = lib.gsvc_unpack_stream(1, ctypes.c_char_p(bytes(buf)), arr, _lib.ptr(dev), _lib.ptr(bound),
                                    None, None, None, 0, p, p, p, None, 65, _lib.ptr(work),
                                    workspace_bytes, None)
        torch.cuda.synchronize()
        return rc

    assert call(v2, len(v1) - 1) == 2 and b"workspace" in lib.gsvc_last_error()
    bad = bytearray(v2)
    bad[242] = 11
    assert call(bad, len(v1)) == 1 and b"prob_bits" in lib.gsvc_last_error()
    assert bool((out == 7.0).all()) and bool((work == 0xa5).all())
