"""CPU: the device encoder's two entries (csrc/ans_enc.hip) as far as they go
without a device -- every refusal with null device pointers (nothing can be
launched), the size query against ans.coded_length, and its per-frame capacity
against the host coder's actual lengths."""
import ctypes

import pytest

import entropy_cases as E
import entropy_encode_cases as X
from gsvc_amd import _lib
from gsvc_amd import ans

BIG = 1 << 40


def encode(sizes, S, capacity=BIG, workspace_bytes=BIG, nframes=None, null_counts=False):
    """gsvc_encode_stream with null device pointers: (status, message)."""
    lib = _lib.load()
    counts = None if null_counts else (ctypes.c_int * max(len(sizes), 1))(*sizes)
    rc = lib.gsvc_encode_stream(len(sizes) if nframes is None else nframes, counts, None, S, None,
                                capacity, None, None, workspace_bytes, None)
    return rc, (lib.gsvc_last_error() if rc else b"")


def test_argument_errors_with_nothing_launched():
    lib = _lib.load()
    for S in (0, 4097, -1):
        rc, msg, _, _ = X.query([300], S)
        assert rc == 1 and b"segment" in msg, (S, msg)
        rc, msg = encode([300], S)
        assert rc == 1 and b"segment" in msg, (S, msg)
    for S in (1, 4096):  # the ends of the range pass the query
        assert X.query([300], S)[0] == 0
    rc, msg, _, _ = X.query([300, -1], 32)
    assert rc == 1 and b"frame 1 has -1 splats" in msg
    rc, msg = encode([300, -1], 32)
    assert rc == 1 and b"frame 1 has -1 splats" in msg
    # 14 N alone passes 2^32: the directory's u32 offsets cannot hold the worst case
    for call in (lambda: X.query([5, 400_000_000], 32)[:2], lambda: encode([5, 400_000_000], 32)):
        rc, msg = call()
        assert rc == 1 and b"u32 offsets" in msg and b"frame 1" in msg
    assert X.query([300_000_000], 4096)[0] == 0  # 4.2e9 + 4 n_seg is still below 2^32
    # an empty list is fine and launches nothing; a negative one and null arrays are not
    rc, _, offs, work = X.query([], 32)
    assert rc == 0 and offs == [0]
    assert encode([], 32) == (0, b"")
    assert encode([], 32, nframes=-1)[0] == 1
    assert encode([300], 32, null_counts=True)[0] == 1 and b"null num_points" in lib.gsvc_last_error()
    counts = (ctypes.c_int * 1)(300)
    assert lib.gsvc_encode_stream_bytes(1, None, 32, None, None) == 1
    assert lib.gsvc_encode_stream_bytes(1, counts, 32, None, None) == 1
    assert b"null coded_offsets" in lib.gsvc_last_error()
    # valid sizes: on to the capacities (status 2), then to the missing device pointers
    _, _, offs, work = X.query([300, 65], 32)
    rc, msg = encode([300, 65], 32, capacity=offs[-1] - 1, workspace_bytes=work)
    assert rc == 2 and b"output" in msg
    rc, msg = encode([300, 65], 32, capacity=offs[-1], workspace_bytes=work - 1)
    assert rc == 2 and b"workspace" in msg
    rc, msg = encode([300, 65], 32, capacity=offs[-1], workspace_bytes=work)
    assert rc == 1 and b"null tensor" in msg


@pytest.mark.parametrize("S", E.SEGMENTS)
def test_size_query_is_coded_length_at_the_worst_case(S):
    sizes = E.SIZES + [50000, 99999]
    rc, _, offs, work = X.query(sizes, S)
    assert rc == 0 and offs[0] == 0
    for f, n in enumerate(sizes):
        n_seg = -(-n // S)
        want = 256 + 1440 + 2 * n + 4 * (n_seg + 1) + 4 * n_seg + 14 * n
        assert want == ans.coded_length(n, n_seg, 4 * n_seg + 14 * n)
        assert offs[f + 1] - offs[f] == X.slot(n, S) and 0 <= X.slot(n, S) - want < 4, (n, S)
    # the workspace holds at least every frame's staged words, and grows with the list
    assert work >= sum(14 * n for n in sizes)
    assert X.query(sizes[:3], S)[3] < work
    assert ans.coded_capacity(sizes, S) == (offs, work)


@pytest.mark.parametrize("S", E.SEGMENTS)
def test_capacity_holds_what_the_host_coder_writes(S):
    streams = [X.stream("case_stream", n, delta) for n in E.SIZES for delta in (False, True)]
    streams += [X.stream(name, *args) for name, args, _ in X.EDGES]
    for s in streams:
        n = X.splats(s)
        rc, _, offs, _ = X.query([n], S)
        assert rc == 0 and len(X.host_coded(s, S)) <= offs[1], (n, S)
