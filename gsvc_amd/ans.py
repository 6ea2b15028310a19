"""The entropy-coded frame stream (version 2): a lossless transcoding of the
fixed-length version-1 stream of compress.py / include/gsvc_amd.h.

Static word-wise rANS (32-bit state, L = 2^16, 16-bit renormalisation, 12-bit
probabilities) over seven symbol channels per splat -- the three Cholesky
codes, the two VQ indices, the high bytes of half(x) and half(y) -- with the
splats cut into segments of S that decode independently; the low bytes of the
positions are stored raw.  DESIGN.md §13 has the layout, the coder and the
normalisation rule.  ``entropy_code`` and ``entropy_expand`` are numpy,
vectorised across segments: one step per symbol position, on all segments at
once.  The device decoder is csrc/ans.hip (``gsvc_expand_stream``); the device
encoder csrc/ans_enc.hip (``gsvc_encode_stream``, here ``entropy_code_device``)
restates ``entropy_code``, which stays the reference its bytes must equal.
"""
from __future__ import annotations

import struct

import numpy as np

STREAM_MAGIC = 0x51565347
STREAM_VERSION = 1
STREAM_VERSION_CODED = 2
HEADER_BYTES = 256
SPLAT_BYTES = 7
EXT_OFFSET = 240               # the 16 bytes version 1 leaves zero
PROB_BITS = 12
PROB_ONE = 1 << PROB_BITS
RANS_L = 1 << 16
MAX_SEGMENT = 4096
ALPHABETS = (64, 64, 64, 8, 8, 256, 256)
CHANNELS = len(ALPHABETS)
TABLE_BYTES = 2 * sum(ALPHABETS)   # 1440
_EXT = struct.Struct("<HHIII")     # S, prob_bits, n_seg, payload_bytes, zero


def coded_length(n: int, n_seg: int, payload_bytes: int) -> int:
    return HEADER_BYTES + TABLE_BYTES + 2 * n + 4 * (n_seg + 1) + payload_bytes


def normalise(counts) -> np.ndarray:
    """Counts of one channel over the frame's N splats -> frequencies that sum
    to 4096: 0 where the count is 0, else max(1, floor(4096 n_s / N)); while
    the sum exceeds 4096 the largest frequency (lowest symbol on ties) loses
    one; the deficit then goes to the largest.  N = 0: f_0 = 4096."""
    counts = np.asarray(counts, np.int64)
    n = int(counts.sum())
    f = np.zeros(counts.shape[0], np.int64)
    if n == 0:
        f[0] = PROB_ONE
        return f
    nz = counts > 0
    f[nz] = np.maximum(1, PROB_ONE * counts[nz] // n)
    while f.sum() > PROB_ONE:
        f[int(np.argmax(f))] -= 1
    f[int(np.argmax(f))] += PROB_ONE - f.sum()
    return f


def _symbols(planes: np.ndarray, n: int):
    """The planes of a version-1 frame -> (symbols [N, 7], low bytes [N, 2])."""
    a = planes[:4 * n].reshape(n, 4)
    b = planes[4 * n:].reshape(n, 3).astype(np.uint32)
    w = b[:, 0] | b[:, 1] << 8 | b[:, 2] << 16
    sym = np.stack([w & 63, (w >> 6) & 63, (w >> 12) & 63, (w >> 18) & 7, (w >> 21) & 7,
                    a[:, 1].astype(np.uint32), a[:, 3].astype(np.uint32)], axis=1).astype(np.int64)
    return sym, np.ascontiguousarray(a[:, [0, 2]])


def _v1_header(buf):
    if len(buf) < HEADER_BYTES:
        raise ValueError(f"stream truncated: {len(buf)} bytes, the header is {HEADER_BYTES}")
    magic, version, n = struct.unpack_from("<IIi", buf, 0)
    if magic != STREAM_MAGIC:
        raise ValueError(f"wrong magic 0x{magic:08x}")
    return version, n


def entropy_code(stream_v1: bytes, segment: int = 32) -> bytes:
    """A version-1 frame stream as a version-2 (entropy-coded) one."""
    s = int(segment)
    if not 1 <= s <= MAX_SEGMENT:
        raise ValueError(f"segment = {segment}, not in 1..{MAX_SEGMENT}")
    version, n = _v1_header(stream_v1)
    if version != STREAM_VERSION:
        raise ValueError(f"stream version {version}, not {STREAM_VERSION}")
    if n < 0 or len(stream_v1) != HEADER_BYTES + SPLAT_BYTES * n:
        raise ValueError(f"stream of {len(stream_v1)} bytes does not hold N = {n} splats")
    if any(stream_v1[EXT_OFFSET:HEADER_BYTES]):
        raise ValueError("bytes 240-255 of a version-1 header are zero")
    sym, low = _symbols(np.frombuffer(stream_v1, np.uint8, offset=HEADER_BYTES), n)
    freq = [normalise(np.bincount(sym[:, c], minlength=a)) for c, a in enumerate(ALPHABETS)]
    start = [np.cumsum(f) - f for f in freq]
    n_seg = -(-n // s)
    # encode: last symbol first, every segment at once; a symbol emits at most one word
    x = np.full(n_seg, RANS_L, np.uint64)
    words = np.zeros((n_seg, CHANNELS * s), np.uint16)
    cnt = np.zeros(n_seg, np.int64)
    first = np.arange(n_seg, dtype=np.int64) * s
    for p in range(s - 1, -1, -1):
        live = np.nonzero(first + p < n)[0]
        if live.size == 0:
            continue
        row = sym[first[live] + p]
        for c in range(CHANNELS - 1, -1, -1):
            f = freq[c][row[:, c]].astype(np.uint64)
            b = start[c][row[:, c]].astype(np.uint64)
            xs = x[live]
            out = xs >= (f << np.uint64(32 - PROB_BITS))  # 64-bit: f may be 4096
            k = live[out]
            words[k, cnt[k]] = (xs[out] & np.uint64(0xffff)).astype(np.uint16)
            cnt[k] += 1
            xs = np.where(out, xs >> np.uint64(16), xs)
            x[live] = ((xs // f) << np.uint64(PROB_BITS)) + xs % f + b
    seg_bytes = 4 + 2 * cnt
    directory = np.zeros(n_seg + 1, np.int64)
    np.cumsum(seg_bytes, out=directory[1:])
    payload_bytes = int(directory[-1])
    if payload_bytes >= 1 << 32:
        raise ValueError("payload does not fit the stream's u32 offsets")
    pay = np.zeros(payload_bytes // 2, np.uint16)
    w0 = directory[:-1] // 2
    pay[w0] = (x & np.uint64(0xffff)).astype(np.uint16)
    pay[w0 + 1] = (x >> np.uint64(16)).astype(np.uint16)
    # the words in reverse order of emission
    e = np.arange(words.shape[1], dtype=np.int64)[None, :]
    used = e < cnt[:, None]
    dest = (w0 + 2 + cnt - 1)[:, None] - e
    pay[dest[used]] = words[used]
    head = bytearray(stream_v1[:HEADER_BYTES])
    struct.pack_into("<I", head, 4, STREAM_VERSION_CODED)
    _EXT.pack_into(head, EXT_OFFSET, s, PROB_BITS, n_seg, payload_bytes, 0)
    tables = np.concatenate(freq).astype("<u2").tobytes()
    out = (bytes(head) + tables + low.tobytes() + directory.astype("<u4").tobytes()
           + pay.astype("<u2").tobytes())
    assert len(out) == coded_length(n, n_seg, payload_bytes)
    return out


def coded_capacity(sizes, segment: int = 32):
    """``gsvc_encode_stream_bytes``: (offsets [F + 1] of the frames' worst-case
    slots in the device encoder's output, its workspace bytes) for frames of
    ``sizes`` splats."""
    import ctypes

    from . import _lib as L
    sizes = [int(n) for n in sizes]
    if any(n >= 1 << 31 for n in sizes):
        raise ValueError("a frame's splat count does not fit the header's i32")
    counts = (ctypes.c_int * max(len(sizes), 1))(*sizes)
    offs = (ctypes.c_longlong * (len(sizes) + 1))()
    work = ctypes.c_size_t(0)
    L.call("gsvc_encode_stream_bytes", len(sizes), counts, int(segment), offs, ctypes.byref(work))
    return list(offs), int(work.value)


def entropy_code_device(frames_v1_dev, sizes, segment: int = 32):
    """``entropy_code`` of every frame of a list on the device
    (``gsvc_encode_stream``, csrc/ans_enc.hip): ``frames_v1_dev`` is a uint8
    tensor on a HIP device holding the concatenated version-1 frames (header and
    planes each), ``sizes`` their splat counts.  One call codes the list; the
    coded lengths are read back once.  Returns the list of coded frames, byte
    for byte what ``entropy_code`` gives for each."""
    import ctypes

    import torch

    from . import _lib as L
    sizes = [int(n) for n in sizes]
    if not sizes:
        return []
    t = frames_v1_dev
    need = sum(HEADER_BYTES + SPLAT_BYTES * max(n, 0) for n in sizes)
    if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.numel() >= need):
        raise ValueError(f"frames_v1_dev is a contiguous uint8 tensor of at least {need} bytes on a HIP device")
    offs, work_bytes = coded_capacity(sizes, segment)
    out = torch.empty((offs[-1],), dtype=torch.uint8, device=t.device)
    lengths = torch.empty((len(sizes),), dtype=torch.int64, device=t.device)
    work = torch.empty((work_bytes,), dtype=torch.uint8, device=t.device)
    counts = (ctypes.c_int * len(sizes))(*sizes)
    L.call("gsvc_encode_stream", len(sizes), counts, L.ptr(t), int(segment), L.ptr(out), out.numel(),
           L.ptr(lengths), L.ptr(work), work.numel(), L.stream(t.device))
    return [out[o:o + n].cpu().numpy().tobytes() for o, n in zip(offs, lengths.cpu().tolist())]


def parse_coded(buf) -> dict:
    """The fields a version-2 frame adds, checked against its length: S, n_seg,
    payload_bytes, the frequency tables and the directory.  ValueError on any
    inconsistency (everything but the payload's own content)."""
    version, n = _v1_header(buf)
    if version != STREAM_VERSION_CODED:
        raise ValueError(f"stream version {version}, not {STREAM_VERSION_CODED}")
    if n < 0:
        raise ValueError(f"N = {n} < 0")
    if struct.unpack_from("<I", buf, 20)[0] & ~1:
        raise ValueError("unknown flags")
    s, prob_bits, n_seg, payload_bytes, zero = _EXT.unpack_from(buf, EXT_OFFSET)
    if not 1 <= s <= MAX_SEGMENT:
        raise ValueError(f"S = {s}, not in 1..{MAX_SEGMENT}")
    if prob_bits != PROB_BITS:
        raise ValueError(f"prob_bits = {prob_bits}, not {PROB_BITS}")
    if n_seg != -(-n // s):
        raise ValueError(f"n_seg = {n_seg}, N = {n} and S = {s} give {-(-n // s)}")
    if zero != 0:
        raise ValueError("reserved header bytes 252-255 are not zero")
    want = coded_length(n, n_seg, payload_bytes)
    if len(buf) != want:
        raise ValueError(f"stream truncated or padded: {len(buf)} bytes, N = {n}, n_seg = {n_seg} "
                         f"and payload_bytes = {payload_bytes} need {want}")
    freq, o = [], HEADER_BYTES
    for c, a in enumerate(ALPHABETS):
        f = np.frombuffer(buf, "<u2", count=a, offset=o).astype(np.int64)
        if int(f.sum()) != PROB_ONE:
            raise ValueError(f"table of channel {c} sums to {int(f.sum())}, not {PROB_ONE}")
        freq.append(f)
        o += 2 * a
    low_off = o
    dir_off = low_off + 2 * n
    d = np.frombuffer(buf, "<u4", count=n_seg + 1, offset=dir_off).astype(np.int64)
    if d[0] != 0 or d[-1] != payload_bytes or (d & 1).any() or (np.diff(d) < 4).any():
        raise ValueError("directory is not 0 .. payload_bytes in even, non-decreasing steps of "
                         "at least one state each")
    return dict(N=n, S=s, n_seg=n_seg, payload_bytes=payload_bytes, freq=freq, directory=d,
                low_offset=low_off, payload_offset=dir_off + 4 * (n_seg + 1))


def entropy_expand(stream_v2: bytes) -> bytes:
    """The version-1 stream a version-2 frame codes, byte for byte; ValueError
    on an inconsistent stream (parse_coded's checks, and each segment's final
    state and word count)."""
    h = parse_coded(stream_v2)
    n, s, n_seg = h["N"], h["S"], h["n_seg"]
    lut = [np.repeat(np.arange(a, dtype=np.int64), f) for a, f in zip(ALPHABETS, h["freq"])]
    start = [np.cumsum(f) - f for f in h["freq"]]
    pay = np.frombuffer(stream_v2, "<u2", count=h["payload_bytes"] // 2,
                        offset=h["payload_offset"]).astype(np.uint64)
    pay = np.append(pay, np.uint64(0))  # what a read past the end gives
    d = h["directory"] // 2
    x = pay[d[:-1]] | pay[d[:-1] + 1] << np.uint64(16)
    wp, we = d[:-1] + 2, d[1:]
    sym = np.zeros((n, CHANNELS), np.int64)
    first = np.arange(n_seg, dtype=np.int64) * s
    for p in range(s):
        live = np.nonzero(first + p < n)[0]
        if live.size == 0:
            break
        for c in range(CHANNELS):
            xs = x[live]
            slot = (xs & np.uint64(PROB_ONE - 1)).astype(np.int64)
            v = lut[c][slot]
            sym[first[live] + p, c] = v
            xs = (h["freq"][c][v].astype(np.uint64) * (xs >> np.uint64(PROB_BITS))
                  + (slot - start[c][v]).astype(np.uint64))
            need = xs < RANS_L
            k = live[need]
            w = pay[np.minimum(wp[k], pay.shape[0] - 1)]
            w[wp[k] >= we[k]] = 0
            xs[need] = xs[need] << np.uint64(16) | w
            wp[k] += 1
            x[live] = xs
    bad = np.nonzero((x != RANS_L) | (wp != we))[0]
    if bad.size:
        k = int(bad[0])
        raise ValueError(f"segment {k} ends in state 0x{int(x[k]):x} after {int(wp[k] - d[k] - 2)} of "
                         f"{int(we[k] - d[k] - 2)} words: the payload is damaged")
    low = np.frombuffer(stream_v2, np.uint8, count=2 * n, offset=h["low_offset"]).reshape(n, 2)
    a = np.stack([low[:, 0], sym[:, 5].astype(np.uint8), low[:, 1], sym[:, 6].astype(np.uint8)], axis=1)
    w = sym[:, 0] | sym[:, 1] << 6 | sym[:, 2] << 12 | sym[:, 3] << 18 | sym[:, 4] << 21
    b = np.stack([w & 0xff, (w >> 8) & 0xff, (w >> 16) & 0xff], axis=1).astype(np.uint8)
    head = bytearray(stream_v2[:HEADER_BYTES])
    struct.pack_into("<I", head, 4, STREAM_VERSION)
    head[EXT_OFFSET:HEADER_BYTES] = bytes(HEADER_BYTES - EXT_OFFSET)
    return bytes(head) + a.tobytes() + b.tobytes()


def channel_bits(stream_v2: bytes) -> dict:
    """Where a version-2 frame's bits go: the ideal cost sum log2(4096 / f) of
    each channel's symbols under the stored tables, and the bytes of the
    header, tables, raw low plane, directory, initial states and words."""
    h = parse_coded(stream_v2)
    sym, _ = _symbols(np.frombuffer(entropy_expand(stream_v2), np.uint8, offset=HEADER_BYTES), h["N"])
    ideal = [float(np.log2(PROB_ONE / f[sym[:, c]]).sum()) for c, f in enumerate(h["freq"])]
    return dict(N=h["N"], ideal_bits=ideal, header_bytes=HEADER_BYTES, table_bytes=TABLE_BYTES,
                low_bytes=2 * h["N"], directory_bytes=4 * (h["n_seg"] + 1),
                state_bytes=4 * h["n_seg"], word_bytes=h["payload_bytes"] - 4 * h["n_seg"])


__all__ = ["entropy_code", "entropy_expand", "entropy_code_device", "coded_capacity", "parse_coded",
           "normalise", "channel_bits",
           "coded_length", "ALPHABETS", "PROB_BITS", "MAX_SEGMENT", "TABLE_BYTES",
           "STREAM_VERSION_CODED"]
