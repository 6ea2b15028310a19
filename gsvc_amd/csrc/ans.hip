// The entropy-coded frame stream (version 2) on gfx950: validation of the host
// copy and the device transcoding back to version-1 bytes.
//
// A version-2 frame is the version-1 header (version = 2, bytes 240-255: u16 S,
// u16 prob_bits = 12, u32 n_seg, u32 payload_bytes, u32 zero), seven u16
// frequency tables (alphabets 64, 64, 64, 8, 8, 256, 256; each sums to 4096),
// the raw low bytes of half(x), half(y) per splat, a directory of n_seg + 1 u32
// payload offsets, and per segment of S splats a u32 rANS state followed by the
// u16 words its decoder consumes.  Decoding a symbol of a channel with
// frequency f and start b:  slot = x & 4095;  s = the symbol whose [b, b + f)
// holds slot;  x = f * (x >> 12) + slot - b;  if (x < 2^16) x = x << 16 | word.
//
// expand_kernel: one lane per (frame, segment), every workgroup serves one
// frame (blockIdx.y).  The workgroup builds the frame's slot tables in LDS --
// one u32 per slot and channel holding the symbol, f - 1 and slot - b, so a
// symbol costs one LDS read -- and each lane then runs its segment's serial
// chain and stores its splats' version-1 plane bytes.  The chain is latency
// bound and the lanes of a wave read and write S splats apart, so a lane works
// in chunks of four splats: one set of 16-byte loads puts the words the chunk
// can consume into a per-lane LDS window (the next word is read beside the slot
// table, off the chain), and the chunk's 28 plane bytes leave as seven dword
// stores where the alignment allows.  The frames' byte ranges
// come from the validated host copy as kernel arguments; everything the kernel
// reads from the device copy (N, S, the tables, the directory) is re-derived
// and clamped against those ranges, so a device copy that differs from the
// host copy cannot make it read or write out of bounds.
#include <vector>

#include "ans.h"

namespace gsvc {

constexpr int kAnsBlock = 256;
constexpr int kExpandFrames = 32;                             // frames per launch
constexpr int kCopyBytesPerLane = 64;                         // a version-1 frame's copy
constexpr int kChunk = 4;                                     // splats decoded per payload window
// a chunk consumes at most 14 * kChunk bytes, from any byte of the first 16-byte line
constexpr int kWindowLines = (14 * kChunk + 15 + 15) / 16;
constexpr int kWindowDwords = 4 * kWindowLines;
constexpr int kWindowStride = kWindowDwords + 1;  // odd: the lanes' windows start in distinct banks

struct ExpandArgs {
    int nframes;
    long long in_off[kExpandFrames + 1];   // frame f: [in_off[f], in_off[f + 1]) of the coded stream
    long long out_off[kExpandFrames + 1];  // and of the expanded one
};

// the window is written as dwords and read as 16-bit words
typedef unsigned __attribute__((may_alias)) window_u32;
typedef unsigned short __attribute__((may_alias)) window_u16;

// slot table entry: symbol | (f - 1) << 8 | (slot - b) << 20
__device__ __forceinline__ unsigned slot_entry(unsigned sym, unsigned f, unsigned j) {
    return sym | (f - 1u) << 8 | j << 20;
}

// The aligned 16 bytes at q, with bytes outside [lo, hi) read as 0.
__device__ __forceinline__ void ld_line(uintptr_t q, uintptr_t lo, uintptr_t hi, unsigned (&v)[4]) {
    if (q >= lo && q + 16 <= hi) {
        const uint4 u = *reinterpret_cast<const uint4 *>(q);
        v[0] = u.x, v[1] = u.y, v[2] = u.z, v[3] = u.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = ld_dword(q + 4 * e, lo, hi);
    }
}

__global__ __launch_bounds__(kAnsBlock) void expand_kernel(ExpandArgs a,
                                                           const unsigned char *__restrict__ in,
                                                           unsigned char *__restrict__ out) {
    __shared__ unsigned lut[kAnsChannels][kProbOne];
    __shared__ unsigned stage[kWindowStride * kAnsBlock];
    const int fr = blockIdx.y;
    if (fr >= a.nframes) return;
    const long long in_len = a.in_off[fr + 1] - a.in_off[fr];
    const long long out_len = a.out_off[fr + 1] - a.out_off[fr];
    if (in_len < kHeaderBytes || out_len < kHeaderBytes) return;
    const unsigned char *src = in + a.in_off[fr];
    unsigned char *dst = out + a.out_off[fr];
    const long long tid = (long long)blockIdx.x * kAnsBlock + threadIdx.x;
    if (rd_u32(src + kOffVersion) != GSVC_STREAM_VERSION_CODED) {  // a version-1 frame: copied
        const long long len = in_len < out_len ? in_len : out_len;
        for (long long i = tid; i < len; i += (long long)gridDim.x * kAnsBlock) dst[i] = src[i];
        return;
    }
    // N, S and the regions they imply, clamped to the frame's two byte ranges
    if (in_len < kCodedFixedBytes) return;
    long long n = (long long)(int)rd_u32(src + kOffN);
    n = n < 0 ? 0 : n;
    n = min(n, (out_len - kHeaderBytes) / kSplatBytes);
    n = min(n, (in_len - kCodedFixedBytes) / 2);
    const int S = min(max((int)rd_u16(src + kOffSegment), 1), kMaxSegment);
    const long long n_seg = (n + S - 1) / S;
    const long long dir_off = kCodedFixedBytes + 2 * n;
    const long long pay_off = dir_off + 4 * (n_seg + 1);
    if (pay_off > in_len) return;
    const long long pay_len = in_len - pay_off;

    if (blockIdx.x == 0)  // the version-1 header
        for (int i = threadIdx.x; i < kHeaderBytes; i += kAnsBlock) {
            unsigned char v = src[i];
            if (i >= kOffVersion && i < kOffVersion + 4) v = i == kOffVersion ? GSVC_STREAM_VERSION : 0;
            if (i >= kOffSegment) v = 0;
            dst[i] = v;
        }

    // Slot tables: a wave per channel.  Lane l holds the channel's symbols
    // l * per ... l * per + per - 1; an inclusive scan over the lanes gives their
    // starts.  Starts and frequencies are clamped to the 4096 slots, and the
    // slots no symbol claims decode as symbol 0 with f = 1.
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = wave; c < kAnsChannels; c += kAnsBlock / 64) {
        const int A = ans_alphabet(c), per = A >= 64 ? A / 64 : 1, owners = A / per;
        const unsigned char *t = src + kHeaderBytes + 2 * ans_first(c);
        unsigned f[4] = {0, 0, 0, 0}, b[4], mine = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < per && lane < owners) {
                f[i] = rd_u16(t + 2 * (lane * per + i));
                mine += f[i];
            }
        unsigned incl = mine;  // at most 256 * 65535
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        unsigned run = incl - mine;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            b[i] = min(run, (unsigned)kProbOne);
            run += f[i];
            f[i] = min(f[i], (unsigned)kProbOne - b[i]);
        }
        // A lane writes the first 64 slots of each of its symbols itself; what a
        // symbol of more than 64 slots has beyond them (at most 63 such symbols)
        // the wave fills together, one symbol at a time.
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < per) {
                const unsigned head = min(f[i], 64u);
                for (unsigned j = 0; j < head; ++j)
                    lut[c][b[i] + j] = slot_entry((unsigned)(lane * per + i), f[i], j);
                unsigned long long more = __ballot(f[i] > 64u);
                while (more) {
                    const int o = __builtin_ctzll(more);
                    more &= more - 1;
                    const unsigned fo = (unsigned)__builtin_amdgcn_readlane((int)f[i], o);
                    const unsigned bo = (unsigned)__builtin_amdgcn_readlane((int)b[i], o);
                    for (unsigned j = 64 + lane; j < fo; j += 64)
                        lut[c][bo + j] = slot_entry((unsigned)(o * per + i), fo, j);
                }
            }
        const unsigned filled = min((unsigned)__builtin_amdgcn_readlane((int)incl, 63), (unsigned)kProbOne);
        for (unsigned j = filled + lane; j < (unsigned)kProbOne; j += 64) lut[c][j] = slot_entry(0, 1, 0);
    }
    __syncthreads();

    const long long k = tid;
    if (k >= n_seg) return;
    const unsigned char *pay = src + pay_off;
    long long d0 = rd_u32(src + dir_off + 4 * k), d1 = rd_u32(src + dir_off + 4 * k + 4);
    d0 = min(d0, pay_len);
    d1 = min(max(d1, d0), pay_len);
    // the segment is pay[d0, d1): a u32 state, then words; past d1 reads as 0
    unsigned x = d0 + 4 <= d1 ? rd_u32(pay + d0) : 0u;
    long long p = d0 + 4;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(src), hi = lo + (uintptr_t)in_len;
    const long long i1 = min((k + 1) * S, n);
    const unsigned char *lowp = src + kCodedFixedBytes;
    unsigned char *pa = dst + kHeaderBytes, *pb = dst + kHeaderBytes + 4 * n;
    // whole chunks leave as dwords when the frame's planes and the segments' starts allow it
    const bool dwords = (reinterpret_cast<uintptr_t>(dst) & 3) == 0 && (S & 3) == 0;
    unsigned char *window = reinterpret_cast<unsigned char *>(stage + threadIdx.x * kWindowStride);
    for (long long i = k * S; i < i1; i += kChunk) {
        const int cnt = (int)min((long long)kChunk, i1 - i);
        // The chunk's splats consume at most 7 * kChunk words: those bytes of the
        // payload, from the 16-byte line that holds pay + p, go to this lane's
        // LDS window, moved down a byte where pay + p is odd, so that a word is
        // one aligned 16-bit read.  Words past the segment's end are zeroed.
        const int avail = p < d1 ? (int)min((d1 - p) >> 1, (long long)(7 * kChunk)) : 0;
        const uintptr_t addr = reinterpret_cast<uintptr_t>(pay) + (uintptr_t)p;
        const uintptr_t base = addr & ~(uintptr_t)15;
        const unsigned at0 = (unsigned)(addr & 14);  // byte of the next word in the window
        unsigned v[kWindowDwords];
#pragma unroll
        for (int j = 0; j < kWindowLines; ++j) ld_line(base + 16 * j, lo, hi, *reinterpret_cast<unsigned(*)[4]>(v + 4 * j));
        if (addr & 1) {
#pragma unroll
            for (int m = 0; m < kWindowDwords; ++m)
                v[m] = v[m] >> 8 | (m + 1 < kWindowDwords ? v[m + 1] << 24 : 0u);
        }
#pragma unroll
        for (int m = 0; m < kWindowDwords; ++m) reinterpret_cast<window_u32 *>(window)[m] = v[m];
        for (int w = avail; w < 7 * kChunk; ++w)
            *reinterpret_cast<window_u16 *>(window + at0 + 2 * w) = 0;
        // the low bytes of the chunk's positions
        const uintptr_t laddr = reinterpret_cast<uintptr_t>(lowp) + (uintptr_t)(2 * i);
        const uintptr_t lq = laddr & ~(uintptr_t)3;
        const unsigned lsh = (unsigned)(laddr & 3) * 8;
        const unsigned l0 = ld_dword(lq, lo, hi), l1 = ld_dword(lq + 4, lo, hi), l2 = ld_dword(lq + 8, lo, hi);
        const unsigned long long low =
            lsh ? ((unsigned long long)l1 << 32 | l0) >> lsh | (unsigned long long)l2 << (64 - lsh)
                : ((unsigned long long)l1 << 32 | l0);
        unsigned at = at0;
        unsigned A[kChunk], B[kChunk];
#pragma unroll
        for (int t = 0; t < kChunk; ++t) {
            A[t] = B[t] = 0;
            if (t < cnt) {
                unsigned sym[kAnsChannels];
#pragma unroll
                for (int c = 0; c < kAnsChannels; ++c) {
                    const unsigned e = lut[c][x & (kProbOne - 1)];
                    const unsigned w = *reinterpret_cast<const window_u16 *>(window + at);
                    sym[c] = e & 0xffu;
                    // f * (x >> 12) + slot - b with f - 1 < 2^12 and x >> 12 < 2^20: one 24-bit mad
                    const unsigned xh = x >> kProbBits;
                    x = __umul24((e >> 8) & 0xfffu, xh) + (xh + (e >> 20));
                    if (x < kRansL) {
                        x = x << 16 | w;
                        at += 2;
                    }
                }
                const unsigned lw = (unsigned)(low >> (16 * t)) & 0xffffu;
                A[t] = (lw & 0xffu) | sym[5] << 8 | (lw >> 8) << 16 | sym[6] << 24;
                // alphabets of 64 and 8 by construction of the tables: the masks cost nothing
                B[t] = (sym[0] & 63u) | (sym[1] & 63u) << 6 | (sym[2] & 63u) << 12 |
                       (sym[3] & 7u) << 18 | (sym[4] & 7u) << 21;
            }
        }
        p += at - at0;
        unsigned char *oa = pa + 4 * i, *ob = pb + 3 * i;
        if (dwords && cnt == kChunk) {
            static_assert(kChunk == 4, "three dwords of plane B per chunk");
            unsigned *wa = reinterpret_cast<unsigned *>(oa), *wb = reinterpret_cast<unsigned *>(ob);
#pragma unroll
            for (int t = 0; t < kChunk; ++t) wa[t] = A[t];
            wb[0] = B[0] | B[1] << 24;
            wb[1] = B[1] >> 8 | B[2] << 16;
            wb[2] = B[2] >> 16 | B[3] << 8;
        } else {
#pragma unroll
            for (int t = 0; t < kChunk; ++t)
                if (t < cnt) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) oa[4 * t + e] = (unsigned char)(A[t] >> (8 * e));
#pragma unroll
                    for (int e = 0; e < 3; ++e) ob[3 * t + e] = (unsigned char)(B[t] >> (8 * e));
                }
        }
    }
}

// What the host copy of a list of frames says, after every check that needs no
// decoding.  prev_points >= 0 adds what spans frames (one H x W, a delta's
// predecessor), as gsvc_unpack_splats checks it.
struct StreamInfo {
    std::vector<long long> expanded;  // num_frames + 1 offsets of the version-1 bytes
    long long total_splats = 0, nmax = 0, max_seg = 0, max_copy = 0;
    bool coded = false;
};

static int validate_frames(const char *who, int num_frames, const unsigned char *stream_host,
                           const long long *frame_offsets, long long prev_points, StreamInfo &info) {
    if (frame_offsets[0] != 0) return set_error(GSVC_ERR_ARG, "%s: frame_offsets[0] != 0", who);
    long long have = prev_points;
    unsigned H = 0, W = 0;
    info.expanded.assign(1, 0);
    for (int f = 0; f < num_frames; ++f) {
        const long long off = frame_offsets[f], len = frame_offsets[f + 1] - off;
        if (len < kHeaderBytes)
            return set_error(GSVC_ERR_ARG, "%s: frame %d truncated (%lld bytes, header is %d)", who, f,
                             len, kHeaderBytes);
        const unsigned char *hdr = stream_host + off;
        if (rd_u32(hdr + kOffMagic) != kStreamMagic)
            return set_error(GSVC_ERR_ARG, "%s: frame %d has a wrong magic 0x%08x", who, f,
                             rd_u32(hdr + kOffMagic));
        const unsigned version = rd_u32(hdr + kOffVersion);
        if (version != GSVC_STREAM_VERSION && version != GSVC_STREAM_VERSION_CODED)
            return set_error(GSVC_ERR_ARG, "%s: frame %d has stream version %u, not %d or %d", who, f,
                             version, GSVC_STREAM_VERSION, GSVC_STREAM_VERSION_CODED);
        const long long n = (long long)(int)rd_u32(hdr + kOffN);
        if (n < 0) return set_error(GSVC_ERR_ARG, "%s: frame %d has N < 0", who, f);
        const unsigned flags = rd_u32(hdr + kOffFlags);
        if (flags & ~1u) return set_error(GSVC_ERR_ARG, "%s: frame %d has unknown flags", who, f);
        if (version == GSVC_STREAM_VERSION) {
            if (len != kHeaderBytes + kSplatBytes * n)
                return set_error(GSVC_ERR_ARG, "%s: frame %d truncated or padded (%lld bytes, "
                                               "N = %lld needs %lld)", who, f, len, n,
                                 kHeaderBytes + kSplatBytes * n);
            info.max_copy = std::max(info.max_copy, len);
        } else {
            const unsigned S = rd_u16(hdr + kOffSegment), prob_bits = rd_u16(hdr + kOffProbBits);
            const long long n_seg = rd_u32(hdr + kOffNumSeg), payload = rd_u32(hdr + kOffPayload);
            if (S < 1 || S > (unsigned)kMaxSegment)
                return set_error(GSVC_ERR_ARG, "%s: frame %d has S = %u, not in 1..%d", who, f, S,
                                 kMaxSegment);
            if (prob_bits != (unsigned)kProbBits)
                return set_error(GSVC_ERR_ARG, "%s: frame %d has prob_bits = %u, not %d", who, f,
                                 prob_bits, kProbBits);
            if (n_seg != (n + S - 1) / S)
                return set_error(GSVC_ERR_ARG, "%s: frame %d has n_seg = %lld, N = %lld and S = %u "
                                               "give %lld", who, f, n_seg, n, S, (n + S - 1) / S);
            if (rd_u32(hdr + kOffReserved) != 0)
                return set_error(GSVC_ERR_ARG, "%s: frame %d has non-zero reserved header bytes", who, f);
            const long long dir_off = kCodedFixedBytes + 2 * n, pay_off = dir_off + 4 * (n_seg + 1);
            if (len != pay_off + payload)
                return set_error(GSVC_ERR_ARG, "%s: frame %d truncated or padded (%lld bytes, N = %lld, "
                                               "n_seg = %lld and payload_bytes = %lld need %lld)", who, f,
                                 len, n, n_seg, payload, pay_off + payload);
            for (int c = 0; c < kAnsChannels; ++c) {
                unsigned sum = 0;
                for (int s = 0; s < ans_alphabet(c); ++s)
                    sum += rd_u16(hdr + kHeaderBytes + 2 * (ans_first(c) + s));
                if (sum != (unsigned)kProbOne)
                    return set_error(GSVC_ERR_ARG, "%s: frame %d: the table of channel %d sums to %u, "
                                                   "not %d", who, f, c, sum, kProbOne);
            }
            // 0 .. payload_bytes in even steps, each holding at least its u32 state
            long long before = 0;
            for (long long k = 0; k <= n_seg; ++k) {
                const long long d = rd_u32(hdr + dir_off + 4 * k);
                const bool ends = k == 0 ? d != 0 : d < before + 4;
                if (ends || (d & 1) || d > payload || (k == n_seg && d != payload))
                    return set_error(GSVC_ERR_ARG, "%s: frame %d: directory entry %lld = %lld is odd, "
                                                   "decreasing, short of a state, or not within the "
                                                   "payload of %lld bytes", who, f, k, d, payload);
                before = d;
            }
            info.coded = true;
            info.max_seg = std::max(info.max_seg, n_seg);
        }
        if (prev_points >= 0) {
            const unsigned h = rd_u32(hdr + kOffH), w = rd_u32(hdr + kOffW);
            if (f == 0) H = h, W = w;
            if (h != H || w != W)
                return set_error(GSVC_ERR_ARG, "%s: frame %d is %ux%u, frame 0 %ux%u", who, f, h, w, H, W);
            if (flags & 1u) {
                if (f == 0 && prev_points == 0)
                    return set_error(GSVC_ERR_ARG, "%s: delta frame %d has no predecessor", who, f);
                if (n > have)
                    return set_error(GSVC_ERR_ARG, "%s: delta frame %d has %lld splats, its "
                                                   "predecessor %lld", who, f, n, have);
            }
        }
        have = n;
        info.total_splats += n;
        info.nmax = std::max(info.nmax, n);
        info.expanded.push_back(info.expanded.back() + kHeaderBytes + kSplatBytes * n);
    }
    return GSVC_OK;
}

static int check_frame_list(const char *who, int num_frames, const unsigned char *stream_host,
                            const long long *frame_offsets) {
    if (num_frames < 0) return set_error(GSVC_ERR_ARG, "%s: num_frames < 0", who);
    if (num_frames > 0 && (!stream_host || !frame_offsets))
        return set_error(GSVC_ERR_ARG, "%s: null stream / frame_offsets", who);
    return GSVC_OK;
}

// the validated frames -> version-1 bytes at expanded_dev, kExpandFrames a launch
static int launch_expand(const char *who, int num_frames, const long long *frame_offsets,
                         const StreamInfo &info, const unsigned char *stream_dev,
                         unsigned char *expanded_dev, hipStream_t s) {
    const long long lanes = std::max(info.max_seg, (info.max_copy + kCopyBytesPerLane - 1) / kCopyBytesPerLane);
    const unsigned blocks = (unsigned)std::max(1ll, (lanes + kAnsBlock - 1) / kAnsBlock);
    for (int f0 = 0; f0 < num_frames; f0 += kExpandFrames) {
        ExpandArgs a;
        a.nframes = std::min(kExpandFrames, num_frames - f0);
        for (int i = 0; i <= kExpandFrames; ++i) {
            const int f = std::min(f0 + i, num_frames);
            a.in_off[i] = frame_offsets[f];
            a.out_off[i] = info.expanded[f];
        }
        hipLaunchKernelGGL(expand_kernel, dim3(blocks, a.nframes), dim3(kAnsBlock), 0, s, a, stream_dev,
                           expanded_dev);
        int rc = check_launch(who);
        if (rc) return rc;
    }
    return GSVC_OK;
}

}  // namespace gsvc

using namespace gsvc;

extern "C" int gsvc_stream_expanded_bytes(int num_frames, const unsigned char *stream_host,
                                          const long long *frame_offsets,
                                          long long *expanded_offsets) {
    int rc = check_frame_list("stream_expanded_bytes", num_frames, stream_host, frame_offsets);
    if (rc) return rc;
    if (!expanded_offsets) return set_error(GSVC_ERR_ARG, "stream_expanded_bytes: null expanded_offsets");
    StreamInfo info;
    info.expanded.assign(1, 0);
    if (num_frames > 0) {
        rc = validate_frames("stream_expanded_bytes", num_frames, stream_host, frame_offsets, -1, info);
        if (rc) return rc;
    }
    for (int f = 0; f <= num_frames; ++f) expanded_offsets[f] = info.expanded[f];
    return GSVC_OK;
}

extern "C" int gsvc_expand_stream(int num_frames, const unsigned char *stream_host,
                                  const long long *frame_offsets, const unsigned char *stream_dev,
                                  unsigned char *expanded_dev, size_t expanded_capacity,
                                  void *stream) {
    int rc = check_frame_list("expand_stream", num_frames, stream_host, frame_offsets);
    if (rc) return rc;
    if (num_frames == 0) return GSVC_OK;
    StreamInfo info;
    rc = validate_frames("expand_stream", num_frames, stream_host, frame_offsets, -1, info);
    if (rc) return rc;
    if ((unsigned long long)info.expanded.back() > (unsigned long long)expanded_capacity)
        return set_error(GSVC_ERR_WORKSPACE, "expand_stream: the expanded stream has %lld bytes, "
                                             "the workspace holds %zu", info.expanded.back(),
                         expanded_capacity);
    if (!stream_dev || !expanded_dev) return set_error(GSVC_ERR_ARG, "expand_stream: null tensor");
    return launch_expand("expand_stream", num_frames, frame_offsets, info, stream_dev, expanded_dev,
                         (hipStream_t)stream);
}

extern "C" int gsvc_unpack_stream(int num_frames, const unsigned char *stream_host,
                                  const long long *frame_offsets, const unsigned char *stream_dev,
                                  const float *cholesky_bound, const float *prev_xyz,
                                  const float *prev_cholesky, const float *prev_features,
                                  int prev_points, float *xq, float *Lq, float *cq, float *Lpre,
                                  long long out_capacity, void *workspace, size_t workspace_bytes,
                                  void *stream) {
    int rc = check_frame_list("unpack_stream", num_frames, stream_host, frame_offsets);
    if (rc) return rc;
    if (num_frames == 0) return GSVC_OK;
    if (prev_points < 0 || (prev_points > 0 && (!prev_xyz || !prev_cholesky || !prev_features)))
        return set_error(GSVC_ERR_ARG, "unpack_stream: bad previous-frame arguments");
    StreamInfo info;
    rc = validate_frames("unpack_stream", num_frames, stream_host, frame_offsets, prev_points, info);
    if (rc) return rc;
    if (info.total_splats > out_capacity)
        return set_error(GSVC_ERR_ARG, "unpack_stream: %lld splats, outputs hold %lld", info.total_splats,
                         out_capacity);
    // a list of version-1 frames alone needs no expansion: the walk reads the stream itself
    const long long bytes = info.expanded.back();
    if (info.coded && (unsigned long long)bytes > (unsigned long long)workspace_bytes)
        return set_error(GSVC_ERR_WORKSPACE, "unpack_stream: the expanded stream has %lld bytes, the "
                                             "workspace holds %zu", bytes, workspace_bytes);
    if (info.total_splats == 0) return GSVC_OK;
    if (!stream_dev || !cholesky_bound || !xq || !Lq || !cq || (info.coded && !workspace))
        return set_error(GSVC_ERR_ARG, "unpack_stream: null tensor");
    hipStream_t s = (hipStream_t)stream;
    const unsigned char *v1 = stream_dev;
    if (info.coded) {
        rc = launch_expand("unpack_stream (expand)", num_frames, frame_offsets, info, stream_dev,
                           (unsigned char *)workspace, s);
        if (rc) return rc;
        v1 = (const unsigned char *)workspace;
    }
    return launch_unpack_walk("unpack_stream", num_frames, v1, bytes, info.total_splats, info.nmax,
                              cholesky_bound, prev_xyz, prev_cholesky, prev_features, prev_points, xq,
                              Lq, cq, Lpre, s);
}
