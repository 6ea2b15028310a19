"""CPU: the entropy-coded stream (gsvc_amd/ans.py, version 2) against the
scalar restatement of tests/entropy_cases.py -- round trips, edge histograms,
bytes and tables, the size bound, the host decoders on mixed lists, and every
refusal of the C entries with null device pointers (nothing can be launched)."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import entropy_cases as E
import quant_cases as Q
from gsvc_amd import ans
from gsvc_amd import compress as C

_streams = {}


def stream(n, delta=False):
    if (n, delta) not in _streams:
        _streams[n, delta] = E.case_stream(n, delta)
    return _streams[n, delta]


def test_case_stream_is_the_models_stream():
    """The restated version-1 stream the tests code is what encode_frame writes."""
    for n, delta in ((65, False), (300, True)):
        m = Q.model_from_case(Q.make_case(n, delta=delta))
        assert C.encode_frame(m) == stream(n, delta)
        for S in (32, 64):
            assert C.encode_frame(m, entropy=True, segment=S) == ans.entropy_code(stream(n, delta), S)
        assert C.encode_frame(m, entropy=True) == ans.entropy_code(stream(n, delta))


@pytest.mark.parametrize("S", E.SEGMENTS)
@pytest.mark.parametrize("n", E.SIZES)
def test_round_trip(n, S):
    """N mod S is 0 for (64, 1), (64, 32), (64, 64), (0, *), (300, 1), ... and
    not for the rest; key and delta frames, and constructed planes."""
    for s in (stream(n), stream(n, True), E.delta_like_stream(n, seed=n)):
        coded = ans.entropy_code(s, S)
        h = C.parse_header(coded)
        assert (h["version"], h["N"], h["S"], h["n_seg"]) == (2, n, S, -(-n // S))
        assert len(coded) == 256 + 1440 + 2 * n + 4 * (h["n_seg"] + 1) + h["payload_bytes"]
        assert len(coded) % 2 == 0
        assert ans.entropy_expand(coded) == s
    assert C.parse_header(stream(n))["version"] == 1
    assert set(C.parse_header(stream(n))) == {"N", "H", "W", "delta", "scale", "beta", "codebooks",
                                              "version"}


def test_edge_histograms():
    const = E.constant_stream(300)
    coded = ans.entropy_code(const, 64)
    _, _, _, _, freq, directory, _ = E.parse(coded)
    assert [max(f) for f in freq] == [4096] * 7  # the 64-bit compare: f << 20 = 2^32
    assert ans.entropy_expand(coded) == const and coded == E.encode(const, 64)
    # f = 4096 costs nothing: every segment is its initial state alone
    assert directory == [4 * k for k in range(6)]

    rare = E.rare_stream()
    coded = ans.entropy_code(rare, 64)
    freq = E.parse(coded)[4]
    assert [sorted(x for x in f if x) for f in freq] == [[1, 4095]] * 7
    assert ans.entropy_expand(coded) == rare

    wide = E.all_bytes_stream()
    coded = ans.entropy_code(wide, 128)
    freq = E.parse(coded)[4]
    assert min(freq[5]) >= 1 and min(freq[6]) >= 1  # all 256 high bytes occur
    assert ans.entropy_expand(coded) == wide


@pytest.mark.parametrize("S", E.SEGMENTS)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 300])
def test_bytes_equal_the_restatement(n, S):
    for s in (stream(n), stream(n, True), E.delta_like_stream(n, seed=n)):
        coded = ans.entropy_code(s, S)
        assert coded == E.encode(s, S)
        syms, _ = E.symbols_of(s)
        freq = E.parse(coded)[4]
        assert freq == E.tables_of(syms)
        for c, f in enumerate(freq):
            assert sum(f) == 4096
            counts = np.bincount([r[c] for r in syms], minlength=len(f)) if n else np.zeros(len(f), int)
            assert all((fs == 0) == (cs == 0) for fs, cs in zip(f, counts)) or n == 0
            assert list(ans.normalise(counts)) == f


def test_restatement_decodes_to_the_end_state():
    """The scalar decoder on entropy_code's bytes: the symbols, x == L and every
    word consumed, segment by segment."""
    s = stream(300, True)
    coded = ans.entropy_code(s, 32)
    n, S, n_seg, _, freq, directory, pay = E.parse(coded)
    start = [[sum(f[:k]) for k in range(len(f))] for f in freq]
    syms, _ = E.symbols_of(s)
    for k in range(n_seg):
        rows, x, used, present = E.decode_segment(coded, pay + directory[k], pay + directory[k + 1],
                                                  min(S, n - k * S), freq, start)
        assert rows == syms[k * S:(k + 1) * S] and x == E.L and used == present


@pytest.mark.parametrize("S", [32, 64, 128])
def test_size(S):
    """32 + 16 words <= sum log2(4096 / f_s) + 33 for every segment: 16 words +
    log2(x_final) = 16 + ideal + eps with x_final >= 2^16, and one bit for the
    floor in x / f."""
    worst = -1e9
    for s in (stream(300), stream(4099, True), E.delta_like_stream(), E.rare_stream(),
              E.constant_stream(300), E.all_bytes_stream()):
        coded = ans.entropy_code(s, S)
        for bits, ideal in E.segment_costs(s, coded):
            worst = max(worst, bits - ideal)
            assert bits <= ideal + 33, (bits, ideal)
    print("S", S, "largest bits over ideal of a segment:", worst)


def test_skewed_stream_is_shorter():
    s = E.delta_like_stream(4099)
    for S in (32, 64, 128):
        coded = ans.entropy_code(s, S)
        print("S", S, "fixed", len(s), "coded", len(coded))
        assert len(coded) < len(s)


def _mixed():
    key = Q.make_case(300)
    ref0 = Q.ref_forward(key)
    d1 = dict(Q.make_case(300, seed=1, delta=True))
    d1["prev"] = (ref0["xq"], ref0["Lpre"], ref0["cq"])
    ref1 = Q.ref_forward(d1)
    d2 = dict(Q.make_case(65, seed=2, delta=True))
    d2["prev"] = tuple(ref1[k][:65] for k in ("xq", "Lpre", "cq"))
    v1 = [C.encode_frame(Q.model_from_case(c)) for c in (key, d1, d2)]
    return v1, [ans.entropy_code(v1[0], 64), v1[1], ans.entropy_code(v1[2], 32)]


def test_host_decode_of_a_mixed_list():
    v1, mixed = _mixed()
    assert [C.parse_header(s)["version"] for s in mixed] == [2, 1, 2]
    want, got = C.unpack_frames_host(v1), C.unpack_frames_host(mixed)
    for a, b in zip(want, got):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    imgs, state = C.decode_frames(v1, "cpu", return_state=True)
    imgs2, state2 = C.decode_frames(mixed, "cpu", return_state=True)
    assert torch.equal(imgs, imgs2) and float(imgs.std()) > 0
    assert all(torch.equal(a, b) for a, b in zip(state, state2))


# ---------------------------------------------------------------- refusals

def _entries(buf, prev_n=0, workspace_bytes=1 << 20, nframes=1, offs=None):
    """The three entries on one host buffer with null device pointers:
    [(status, message)] of gsvc_stream_expanded_bytes, gsvc_expand_stream,
    gsvc_unpack_stream."""
    from gsvc_amd import _lib
    lib = _lib.load()
    buf = bytes(buf)
    offs = offs or [0, len(buf)]
    arr = (ctypes.c_longlong * len(offs))(*offs)
    exp = (ctypes.c_longlong * len(offs))()
    host = ctypes.c_char_p(buf)
    out = []
    for call in (lambda: lib.gsvc_stream_expanded_bytes(nframes, host, arr, exp),
                 lambda: lib.gsvc_expand_stream(nframes, host, arr, None, None, workspace_bytes, None),
                 lambda: lib.gsvc_unpack_stream(nframes, host, arr, None, None, None, None, None, prev_n,
                                                None, None, None, None, 1 << 20, None, workspace_bytes,
                                                None)):
        rc = call()
        out.append((rc, lib.gsvc_last_error() if rc else b""))
    return out


def _put(buf, fmt, off, *vals):
    b = bytearray(buf)
    struct.pack_into(fmt, b, off, *vals)
    return bytes(b)


def _corruptions(good):
    """(name, bytes, word the C message names) of one-field corruptions of a
    valid version-2 frame of N = 300, S = 64."""
    n, S, n_seg, payload, _, directory, pay = E.parse(good)
    d = pay - 4 * (n_seg + 1)
    table0 = bytearray(good)
    f0 = list(struct.unpack_from("<64H", good, 256))
    k = f0.index(max(f0))
    struct.pack_into("<H", table0, 256 + 2 * k, f0[k] - 1)  # channel 0 sums to 4095
    return [
        ("S = 0", _put(good, "<H", 240, 0), b"S = 0"),
        ("S > 4096", _put(good, "<H", 240, 4097), b"S = 4097"),
        ("prob_bits", _put(good, "<H", 242, 11), b"prob_bits"),
        ("n_seg", _put(good, "<I", 244, n_seg + 1), b"n_seg"),
        ("table", bytes(table0), b"table of channel 0 sums to 4095"),
        ("directory odd", _put(good, "<I", d + 8, directory[2] + 1), b"directory"),
        ("directory decreasing", _put(good, "<I", d + 8, directory[1] - 2), b"directory"),
        ("directory past the payload", _put(good, "<I", d + 12, payload + 2), b"directory"),
        ("truncated", good[:-2], b"truncated or padded"),
        ("padded", good + b"\0\0", b"truncated or padded"),
        ("flags", _put(good, "<I", 20, 2), b"flags"),
    ]


def test_refusals_with_nothing_launched():
    from gsvc_amd import _lib
    lib = _lib.load()
    good = ans.entropy_code(stream(300), 64)
    n_exp = 256 + 7 * 300
    # a valid frame passes validation: the first entry succeeds, the other two
    # stop at the missing device pointers
    (r0, _), (r1, m1), (r2, m2) = _entries(good)
    assert r0 == 0 and r1 == 1 and r2 == 1 and b"null tensor" in m1 and b"null tensor" in m2
    for name, bad, word in _corruptions(good):
        for rc, msg in _entries(bad):
            assert rc == 1 and word in msg, (name, rc, msg)
        with pytest.raises(ValueError):
            ans.entropy_expand(bad)
        with pytest.raises(ValueError):
            C.unpack_frames_host([bad])
    # what spans frames is gsvc_unpack_stream's to check: it alone knows the predecessor
    delta = ans.entropy_code(stream(300, True), 64)
    (r0, _), (r1, m1), (r2, m2) = _entries(delta)
    assert r0 == 0 and b"null tensor" in m1 and r2 == 1 and b"no predecessor" in m2
    assert _entries(delta, prev_n=3)[2][1].find(b"previous-frame") >= 0
    # a workspace that is too small: status 2, from the two entries that take one
    (r0, _), (r1, m1), (r2, m2) = _entries(good, workspace_bytes=n_exp - 1)
    assert r0 == 0 and r1 == 2 and r2 == 2 and b"workspace" in m1 and b"workspace" in m2
    assert _entries(good, workspace_bytes=n_exp)[1][0] == 1  # large enough: on to the null pointers
    # gsvc_unpack_splats keeps refusing version 2
    arr = (ctypes.c_longlong * 2)(0, len(good))
    assert lib.gsvc_unpack_splats(1, ctypes.c_char_p(good), arr, None, None, None, None, None, 0, None,
                                  None, None, None, 1 << 20, None) == 1
    assert b"stream version" in lib.gsvc_last_error()
    # the offsets of a mixed list, and an empty one
    v1 = stream(65)
    blob = v1 + good + v1
    offs = [0, len(v1), len(v1) + len(good), len(blob)]
    arr = (ctypes.c_longlong * 4)(*offs)
    exp = (ctypes.c_longlong * 4)()
    assert lib.gsvc_stream_expanded_bytes(3, ctypes.c_char_p(blob), arr, exp) == 0
    assert list(exp) == [0, len(v1), len(v1) + n_exp, 2 * len(v1) + n_exp]
    assert lib.gsvc_stream_expanded_bytes(0, None, None, exp) == 0 and exp[0] == 0
    assert lib.gsvc_stream_expanded_bytes(-1, None, None, exp) == 1
    assert lib.gsvc_expand_stream(1, None, None, None, None, 0, None) == 1


def test_flip_sweep_of_header_extension_and_directory():
    """Every single byte of the 16 header-extension bytes and of the directory,
    complemented: all three entries refuse it, and so does the host decoder."""
    good = ans.entropy_code(stream(300), 64)
    n, S, n_seg, payload, _, directory, pay = E.parse(good)
    assert n_seg == 5
    spots = list(range(240, 256)) + list(range(pay - 4 * (n_seg + 1), pay))
    for o in spots:
        bad = bytearray(good)
        bad[o] ^= 0xff
        for rc, msg in _entries(bad):
            assert rc != 0 and msg, (o, rc)
        with pytest.raises(ValueError):
            ans.entropy_expand(bytes(bad))


def test_damaged_payload_trips_the_final_state():
    good = ans.entropy_code(stream(300), 64)
    pay = E.parse(good)[6]
    directory = E.parse(good)[5]
    for o in (pay + 4, pay + directory[2] + 6, len(good) - 2):  # one word each
        bad = bytearray(good)
        bad[o] ^= 0xff
        bad[o + 1] ^= 0xff
        with pytest.raises(ValueError, match="damaged"):
            ans.entropy_expand(bytes(bad))
    with pytest.raises(ValueError, match="segment"):
        ans.entropy_code(stream(5), 0)
    with pytest.raises(ValueError, match="segment"):
        ans.entropy_code(stream(5), 4097)
    with pytest.raises(ValueError, match="version"):
        ans.entropy_code(good, 64)


def test_compress_video_keys_without_entropy_cpu():
    """entropy=False returns exactly the keys it always did; entropy=True adds
    bpp_coded and version-2 streams (CPU dispatch, one tiny frame, no training
    steps: the optimizer is a device kernel)."""
    from gsvc_amd.frame import synthetic_gt
    torch.manual_seed(3)
    frames = [synthetic_gt(E.H, E.W, 1, "cpu")]
    sd = {"frame_1": {"_xyz": torch.atanh(2 * (torch.rand(33, 2) - 0.5)),
                      "_cholesky": 3 * torch.rand(33, 3), "_features_dc": torch.rand(33, 3)}}
    plain = C.compress_video(sd, frames, iterations=0, device="cpu", seed=0)
    assert set(plain) == {"streams", "psnr", "bpp", "bpp_entropy_estimate", "state_dicts"}
    coded = C.compress_video(sd, frames, iterations=0, device="cpu", seed=0, entropy=True, segment=32)
    assert set(coded) == set(plain) | {"bpp_coded"}
    assert C.parse_header(coded["streams"][0])["version"] == 2
    assert coded["bpp_coded"] == [8 * len(coded["streams"][0]) / E.H / E.W]
    assert ans.entropy_expand(coded["streams"][0]) == plain["streams"][0]
