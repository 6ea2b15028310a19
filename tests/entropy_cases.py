"""Inputs and the scalar restatement shared by test_entropy_cpu.py and
test_entropy_gpu.py.  The restatement is the coded stream (version 2) of
DESIGN.md §13 in plain Python loops, one symbol at a time; it imports nothing
from the package under test."""
import math
import struct

import numpy as np

import quant_cases as Q

ALPHABETS = (64, 64, 64, 8, 8, 256, 256)
L = 1 << 16
SIZES = [0, 1, 63, 64, 65, 300, 4099]
SEGMENTS = [1, 32, 64, 128, 4096]
H, W = 40, 72


# ---------------------------------------------------------------- version-1 streams

def v1_header(n, delta=False, h=H, w=W):
    """A version-1 header restated: magic, version, N, H, W, flags, the test
    quantizer's tables, zero to byte 256."""
    vals = list(Q.SCALE) + list(Q.BETA) + list(Q.codebooks().reshape(-1))
    head = struct.pack("<IIiIII54f", 0x51565347, 1, n, h, w, 1 if delta else 0, *map(float, vals))
    return head + bytes(256 - len(head))


def v1_stream(half_bits, codes_chol, codes_rgb, delta=False):
    """A version-1 frame from the positions' half bit patterns [N, 2] (uint16)
    and the codes."""
    n = half_bits.shape[0]
    cc, cr = codes_chol.astype(np.uint32), codes_rgb.astype(np.uint32)
    w = cc[:, 0] | cc[:, 1] << 6 | cc[:, 2] << 12 | cr[:, 0] << 18 | cr[:, 1] << 21
    b = np.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255], 1).astype(np.uint8)
    return v1_header(n, delta) + half_bits.astype("<u2").tobytes() + b.tobytes()


def case_stream(n, delta=False, seed=0):
    """The stream of quant_cases.make_case's model, from the restated forward."""
    if n == 0:
        return v1_header(0, delta)
    case = Q.make_case(n, seed=seed, delta=delta)
    ref = Q.ref_forward(case)
    half = case["xyz"].astype(np.float16).view(np.uint16)
    return v1_stream(half, ref["codes_chol"], ref["codes_rgb"], delta)


def constant_stream(n):
    """Every splat carries the same codes and position: one symbol per channel
    has f = 4096."""
    return v1_stream(np.full((n, 2), 0x3c00, np.uint16), np.full((n, 3), 17, np.uint8),
                     np.full((n, 2), 5, np.uint8))


def rare_stream(n=4099):
    """One rare symbol among n - 1 others in every channel: its f is 1."""
    half = np.full((n, 2), 0x3555, np.uint16)
    cc = np.full((n, 3), 40, np.uint8)
    cr = np.full((n, 2), 2, np.uint8)
    half[n // 3] = [0xb7aa, 0x0001]
    cc[n // 3] = [0, 63, 1]
    cr[n // 3] = [7, 0]
    return v1_stream(half, cc, cr)


def all_bytes_stream(n=4099, seed=3):
    """Position high bytes that span all 256 values."""
    rng = np.random.default_rng(seed)
    half = rng.integers(0, 1 << 16, (n, 2)).astype(np.uint16)
    half[:256, 0] = np.arange(256) << 8 | 0x5a
    half[-256:, 1] = np.arange(255, -1, -1) << 8
    return v1_stream(half, rng.integers(0, 64, (n, 3)).astype(np.uint8),
                     rng.integers(0, 8, (n, 2)).astype(np.uint8))


def delta_like_stream(n=4099, seed=4, delta=True):
    """Codes as a delta frame has them: Cholesky codes and colour indices peaked
    on a few values, position deltas small (high bytes of a few exponents)."""
    rng = np.random.default_rng(seed)
    cc = np.clip(np.rint(rng.normal(31, 1.2, (n, 3))), 0, 63).astype(np.uint8)
    cr = np.where(rng.random((n, 2)) < 0.85, 3, rng.integers(0, 8, (n, 2))).astype(np.uint8)
    xy = (rng.normal(0, 0.004, (n, 2))).astype(np.float16).view(np.uint16)
    return v1_stream(xy, cc, cr, delta)


# ---------------------------------------------------------------- the coder, restated

def symbols_of(stream_v1):
    """([N][7] symbols, [N][2] low bytes) of a version-1 stream."""
    n = struct.unpack_from("<i", stream_v1, 8)[0]
    syms, lows = [], []
    for i in range(n):
        xl, xh, yl, yh = stream_v1[256 + 4 * i:260 + 4 * i]
        o = 256 + 4 * n + 3 * i
        w = stream_v1[o] | stream_v1[o + 1] << 8 | stream_v1[o + 2] << 16
        syms.append([w & 63, (w >> 6) & 63, (w >> 12) & 63, (w >> 18) & 7, (w >> 21) & 7, xh, yh])
        lows.append([xl, yl])
    return syms, lows


def normalise(counts):
    n = sum(counts)
    if n == 0:
        return [4096] + [0] * (len(counts) - 1)
    f = [0 if c == 0 else max(1, 4096 * c // n) for c in counts]
    while sum(f) > 4096:
        f[f.index(max(f))] -= 1      # index(): the lowest symbol of the largest
    f[f.index(max(f))] += 4096 - sum(f)
    return f


def tables_of(syms):
    freq = []
    for c, a in enumerate(ALPHABETS):
        counts = [0] * a
        for row in syms:
            counts[row[c]] += 1
        freq.append(normalise(counts))
    return freq


def encode_segment(rows, freq, start):
    """(final state, words in decoding order) of one segment's symbol rows."""
    x, words = L, []
    for row in reversed(rows):
        for c in range(6, -1, -1):
            f, b = freq[c][row[c]], start[c][row[c]]
            if x >= f << 20:
                words.append(x & 0xffff)
                x >>= 16
            x = ((x // f) << 12) + x % f + b
    return x, words[::-1]


def encode(stream_v1, S):
    """entropy_code restated."""
    syms, lows = symbols_of(stream_v1)
    n = len(syms)
    freq = tables_of(syms)
    start = [[sum(f[:s]) for s in range(len(f))] for f in freq]
    segs = [encode_segment(syms[k:k + S], freq, start) for k in range(0, n, S)]
    payload, directory = b"", [0]
    for x, words in segs:
        payload += struct.pack("<I", x) + struct.pack(f"<{len(words)}H", *words)
        directory.append(len(payload))
    head = bytearray(stream_v1[:256])
    struct.pack_into("<I", head, 4, 2)
    struct.pack_into("<HHIII", head, 240, S, 12, len(segs), len(payload), 0)
    out = bytes(head)
    for f in freq:
        out += struct.pack(f"<{len(f)}H", *f)
    out += bytes(b for low in lows for b in low)
    out += struct.pack(f"<{len(directory)}I", *directory)
    return out + payload


def parse(stream_v2):
    """(N, S, n_seg, payload_bytes, freq, directory, payload offset) of a
    version-2 stream, unchecked."""
    n = struct.unpack_from("<i", stream_v2, 8)[0]
    S, _, n_seg, payload_bytes, _ = struct.unpack_from("<HHIII", stream_v2, 240)
    freq, o = [], 256
    for a in ALPHABETS:
        freq.append(list(struct.unpack_from(f"<{a}H", stream_v2, o)))
        o += 2 * a
    o += 2 * n
    directory = list(struct.unpack_from(f"<{n_seg + 1}I", stream_v2, o))
    return n, S, n_seg, payload_bytes, freq, directory, o + 4 * (n_seg + 1)


def decode_segment(stream_v2, lo, hi, count, freq, start):
    """count splats of the segment at bytes [lo, hi): (rows, final state, words
    consumed, words present)."""
    x = struct.unpack_from("<I", stream_v2, lo)[0]
    words = struct.unpack_from(f"<{(hi - lo - 4) // 2}H", stream_v2, lo + 4)
    used, rows = 0, []
    for _ in range(count):
        row = []
        for c in range(7):
            slot = x & 4095
            s = next(s for s in range(len(freq[c])) if start[c][s] <= slot < start[c][s] + freq[c][s])
            row.append(s)
            x = freq[c][s] * (x >> 12) + slot - start[c][s]
            if x < L:
                x = x << 16 | (words[used] if used < len(words) else 0)
                used += 1
        rows.append(row)
    return rows, x, used, len(words)


def segment_costs(stream_v1, stream_v2):
    """Per segment (32 + 16 words, sum log2(4096 / f_s) of its symbols)."""
    syms, _ = symbols_of(stream_v1)
    n, S, n_seg, _, freq, directory, _ = parse(stream_v2)
    out = []
    for k in range(n_seg):
        ideal = sum(math.log2(4096 / freq[c][row[c]]) for row in syms[k * S:(k + 1) * S] for c in range(7))
        out.append((8 * (directory[k + 1] - directory[k]), ideal))
    return out
