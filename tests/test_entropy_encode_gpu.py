"""GPU: the device encoder of the entropy-coded stream (csrc/ans_enc.hip,
gsvc_encode_stream) against the host coder ans.entropy_code, byte for byte."""
import ctypes

import numpy as np
import pytest
import torch

import entropy_cases as E
import entropy_encode_cases as X
import quant_cases as Q
from gsvc_amd import _lib
from gsvc_amd import ans
from gsvc_amd import compress as C

pytestmark = pytest.mark.gpu

H, W = E.H, E.W
GUARD = 64


def device_code(streams, S, shift=0):
    """gsvc_encode_stream on the concatenated version-1 frames: (each frame's
    coded bytes, the reported lengths).  The output is GUARD bytes longer than
    the query's capacity and filled with 0xa5, as are the lengths and the
    workspace: nothing past the capacity may change and nothing may rely on a
    zeroed workspace.  ``shift`` moves both the input and the output off their
    allocations' alignment by that many bytes."""
    sizes = [X.splats(s) for s in streams]
    offs, work_bytes = ans.coded_capacity(sizes, S)
    blob = bytes(shift) + b"".join(streams)
    dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    out = torch.full((shift + offs[-1] + GUARD,), 0xa5, dtype=torch.uint8, device="cuda")
    lengths = torch.full((len(streams),), -1, dtype=torch.int64, device="cuda")
    work = torch.full((work_bytes,), 0xa5, dtype=torch.uint8, device="cuda")
    counts = (ctypes.c_int * len(sizes))(*sizes)
    _lib.call("gsvc_encode_stream", len(sizes), counts, ctypes.c_void_p(dev.data_ptr() + shift), S,
              ctypes.c_void_p(out.data_ptr() + shift), offs[-1], _lib.ptr(lengths), _lib.ptr(work),
              work_bytes, _lib.stream(out.device))
    got = out.cpu().numpy().tobytes()
    assert got[:shift] == b"\xa5" * shift and got[shift + offs[-1]:] == b"\xa5" * GUARD
    lens = lengths.cpu().tolist()
    assert all(0 < n <= b - a for n, a, b in zip(lens, offs, offs[1:])), (lens, offs)
    return [got[shift + o:shift + o + n] for o, n in zip(offs, lens)], lens


def check(streams, S, shift=0):
    got, lens = device_code(streams, S, shift)
    for f, s in enumerate(streams):
        want = X.host_coded(s, S)
        assert lens[f] == len(want), (f, lens[f], len(want))
        assert got[f] == want, (f, X.splats(s), S)
    return got


@pytest.mark.parametrize("S", E.SEGMENTS)
@pytest.mark.parametrize("n", E.SIZES)
def test_bytes_equal_the_host_coders(cuda, n, S):
    """The empty frame, one splat, tails one short of, equal to and one past S,
    one segment for the whole frame; key and delta frames."""
    for delta in (False, True):
        check([X.stream("case_stream", n, delta)], S)


def test_edge_histograms(cuda):
    """f = 4096 (the 64-bit compare; no word at all), f = 1, all 256 high bytes,
    peaked delta-like codes."""
    for name, args, S in X.EDGES:
        got = check([X.stream(name, *args)], S)
        if name == "constant_stream":  # five segments of a state each
            assert len(got[0]) == 256 + 1440 + 600 + 4 * 6 + 4 * 5


def test_normalisation_corners(cuda):
    """Each stream first shown, on the host, to take the branch it is named for."""
    c = X.channel5_counts(X.stream("corner_excess"))
    raw = X.floors(c)
    assert sum(raw) == 4340 and sorted(raw)[-2:] == [1, 4085]
    f = list(ans.normalise(c))
    assert f == E.normalise(list(c)) and f[200] == 4085 - 244 and sum(f) == 4096

    c = X.channel5_counts(X.stream("corner_tie"))
    raw = X.floors(c)
    assert raw[7] == raw[9] == 2007 and sum(raw) == 4215
    f = list(ans.normalise(c))
    assert f == E.normalise(list(c)) and (f[7], f[9]) == (1947, 1948)  # the lowest lost first

    c = X.channel5_counts(X.stream("corner_deficit"))
    raw = X.floors(c)
    assert sum(raw) == 4095 and raw[10] == raw[20] == raw[30] == 1365
    f = list(ans.normalise(c))
    assert f == E.normalise(list(c)) and (f[10], f[20], f[30]) == (1366, 1365, 1365)

    for name in ("corner_excess", "corner_tie", "corner_deficit"):
        check([X.stream(name)], 64)


def test_lists(cuda):
    """Eight frames in one call, N mixed with 0, 1 and odd counts so that later
    frames start at odd input offsets; the same with input and output moved one
    byte off; F = 1; 35 frames, more than one launch takes."""
    frames = [X.stream("case_stream", n, delta) for n, delta in
              ((63, False), (300, True), (0, False), (1, True), (65, False), (4099, True), (64, False),
               (301, True))]
    assert len(frames[0]) % 2 == 1 and len(b"".join(frames[:3])) % 2 == 1  # frames 1, 2, 3 start odd
    for S in (32, 128):
        check(frames, S)
    check(frames, 64, shift=1)
    check(frames[1:4], 1, shift=3)
    check([frames[5]], 32)
    check([frames[k % 5] for k in range(35)], 32)


def expand_on_device(streams):
    """gsvc_expand_stream on the concatenated coded frames, read back."""
    blob = b"".join(streams)
    offs = [0]
    for s in streams:
        offs.append(offs[-1] + len(s))
    arr = (ctypes.c_longlong * len(offs))(*offs)
    exp = (ctypes.c_longlong * len(offs))()
    _lib.call("gsvc_stream_expanded_bytes", len(streams), ctypes.c_char_p(blob), arr, exp)
    dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    out = torch.empty((exp[len(streams)],), dtype=torch.uint8, device="cuda")
    _lib.call("gsvc_expand_stream", len(streams), ctypes.c_char_p(blob), arr, _lib.ptr(dev), _lib.ptr(out),
              out.numel(), _lib.stream(out.device))
    return out.cpu().numpy().tobytes()


def test_round_trip_on_the_device(cuda):
    frames = [X.stream("case_stream", 300, False), X.stream("delta_like_stream"),
              X.stream("case_stream", 65, True), X.stream("constant_stream", 300)]
    for S in (32, 4096):
        got, _ = device_code(frames, S)
        assert expand_on_device(got) == b"".join(frames)


def test_public_path(cuda):
    """encode_frame / encode_frames of models on the device: the host coder's
    bytes, the list equal to the single encodes, two runs equal, and the decode
    of the coded list equal to the decode of the version-1 list."""
    key = Q.make_case(300)
    ref0 = Q.ref_forward(key)
    d1 = dict(Q.make_case(300, seed=1, delta=True))
    d1["prev"] = (ref0["xq"], ref0["Lpre"], ref0["cq"])
    ref1 = Q.ref_forward(d1)
    d2 = dict(Q.make_case(65, seed=2, delta=True))
    d2["prev"] = tuple(ref1[k][:65] for k in ("xq", "Lpre", "cq"))
    models = [Q.model_from_case(c, H, W, device="cuda") for c in (key, d1, d2)]
    v1 = [C.encode_frame(m) for m in models]
    assert v1 == C.encode_frames(models) and [len(s) for s in v1] == [256 + 7 * n for n in (300, 300, 65)]
    assert v1 == [C.encode_frame(Q.model_from_case(c, H, W)) for c in (key, d1, d2)]  # CPU models
    for S in (32, 64, 4096):
        single = [C.encode_frame(m, entropy=True, segment=S) for m in models]
        assert single == [X.host_coded(s, S) for s in v1]
        assert C.encode_frames(models, entropy=True, segment=S) == single
        assert C.encode_frames(models, entropy=True, segment=S) == single  # two runs
    assert C.encode_frame(models[1], entropy=True) == X.host_coded(v1[1], 32)
    assert ans.entropy_code_device(torch.frombuffer(bytearray(b"".join(v1)), dtype=torch.uint8).cuda(),
                                   [300, 300, 65], 64) == [X.host_coded(s, 64) for s in v1]
    with pytest.raises(ValueError, match="segment"):
        C.encode_frame(models[0], entropy=True, segment=0)
    coded = C.encode_frames(models, entropy=True)
    assert torch.equal(C.decode_frames(coded, "cuda"), C.decode_frames(v1, "cuda"))


def test_short_buffers_launch_nothing(cuda):
    """A workspace or an output capacity one byte short: status 2, and the
    output and the lengths keep their fill."""
    lib = _lib.load()
    s = X.stream("case_stream", 65, False)
    offs, work_bytes = ans.coded_capacity([65], 32)
    dev = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
    out = torch.full((offs[-1],), 0xa5, dtype=torch.uint8, device="cuda")
    lengths = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    work = torch.empty((work_bytes,), dtype=torch.uint8, device="cuda")
    counts = (ctypes.c_int * 1)(65)
    for capacity, workspace, word in ((offs[-1] - 1, work_bytes, b"output"), (offs[-1], work_bytes - 1, b"workspace")):
        rc = lib.gsvc_encode_stream(1, counts, _lib.ptr(dev), 32, _lib.ptr(out), capacity, _lib.ptr(lengths),
                                    _lib.ptr(work), workspace, None)
        torch.cuda.synchronize()
        assert rc == 2 and word in lib.gsvc_last_error()
        assert bool((out == 0xa5).all()) and int(lengths[0]) == -1
