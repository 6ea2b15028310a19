"""What test_entropy_encode_cpu.py and test_entropy_encode_gpu.py share: the
host coder's bytes computed once per (stream, S), the streams that drive each
branch of the normalisation, and the raw calls of the two encoder entries."""
import ctypes
import struct

import numpy as np

import entropy_cases as E
from gsvc_amd import _lib
from gsvc_amd import ans

_streams, _coded = {}, {}


def stream(name, *args):
    """A version-1 stream by the name of its maker in entropy_cases (or
    ``corner_*`` here), built once."""
    k = (name,) + args
    if k not in _streams:
        _streams[k] = (globals().get(name) or getattr(E, name))(*args)
    return _streams[k]


def host_coded(s, S):
    """ans.entropy_code(s, S), computed once."""
    k = (s, S)
    if k not in _coded:
        _coded[k] = ans.entropy_code(s, S)
    return _coded[k]


def splats(s):
    return struct.unpack_from("<i", s, 8)[0]


EDGES = (("constant_stream", (300,), 64), ("rare_stream", (), 64), ("all_bytes_stream", (), 128),
         ("delta_like_stream", (), 32))


# ---------------------------------------------------------------- normalisation corners

def _corner(high_x, seed):
    """A version-1 stream whose channel 5 (the high byte of half(x)) holds
    ``high_x``; the other channels are random."""
    n = len(high_x)
    rng = np.random.default_rng(seed)
    half = rng.integers(0, 1 << 16, (n, 2)).astype(np.uint16)
    half[:, 0] = (half[:, 0] & 0xff) | np.asarray(high_x, np.uint16) << 8
    return E.v1_stream(half, rng.integers(0, 64, (n, 3)).astype(np.uint8),
                       rng.integers(0, 8, (n, 2)).astype(np.uint8))


def corner_excess():
    """255 symbols seen once and symbol 200 the other 99 745 times, N = 100 000:
    255 + floor(4096 * 99745 / 100000) = 4340, so the largest loses 244."""
    sym = np.full(100000, 200, np.int64)
    rare = [s for s in range(256) if s != 200]
    sym[np.arange(255) * 391 + 5] = rare
    return _corner(sym, 11)


def corner_tie():
    """Symbols 7 and 9 seen 5000 times each and 201 others once, N = 10 201:
    2 * 2007 + 201 = 4215, an odd excess of 119 that the two take turns to lose
    from: the lower symbol goes first, so it ends one below the higher."""
    sym = np.concatenate([np.full(5000, 7), np.full(5000, 9), 20 + np.arange(201)])
    return _corner(np.random.default_rng(12).permutation(sym), 13)


def corner_deficit():
    """Three symbols 1000 times each: 3 * 1365 = 4095, the lowest gets the one."""
    return _corner(np.tile([30, 10, 20], 1000), 14)


def channel5_counts(s):
    n = splats(s)
    return np.bincount(np.frombuffer(s, np.uint8, 4 * n, 256)[1::4], minlength=256)


def floors(counts):
    """max(1, floor(4096 n_s / N)) of the symbols that occur, before any correction."""
    n = int(sum(counts))
    return [0 if c == 0 else max(1, 4096 * int(c) // n) for c in counts]


# ---------------------------------------------------------------- the entries, raw

def query(sizes, S):
    """gsvc_encode_stream_bytes: (status, message, offsets [F + 1], workspace bytes)."""
    lib = _lib.load()
    counts = (ctypes.c_int * max(len(sizes), 1))(*sizes)
    offs = (ctypes.c_longlong * (len(sizes) + 1))()
    work = ctypes.c_size_t(0)
    rc = lib.gsvc_encode_stream_bytes(len(sizes), counts, S, offs, ctypes.byref(work))
    return rc, (lib.gsvc_last_error() if rc else b""), list(offs), int(work.value)


def slot(n, S):
    """What the size query must give a frame of n splats: ans.coded_length with
    every symbol emitting a word, rounded up to the slot alignment of 4."""
    n_seg = -(-n // S)
    return -(-ans.coded_length(n, n_seg, 4 * n_seg + 14 * n) // 4) * 4
