// The encoder of the entropy-coded frame stream (version 2) on gfx950: F
// concatenated version-1 frames in device memory -> the bytes
// gsvc_amd.ans.entropy_code gives for each (DESIGN.md §13b "Encoder").  Integer
// arithmetic throughout, no atomics across workgroups; equal inputs give equal
// bytes.
//
// Four kernels per launch of up to 32 frames (blockIdx.y, or blockIdx.x where a
// workgroup serves a whole frame):
//   enc_hist_kernel    a workgroup per 2048 splats: an LDS histogram of the seven
//                      channels (integer LDS atomics), stored as the workgroup's
//                      own partial histogram; copies the raw low-byte plane.
//   enc_tables_kernel  one workgroup per frame, a wave per channel: the partial
//                      histograms summed in block order, ans.normalise restated
//                      (long division for 4096 n_s / N, the excess taken off the
//                      top levels all at once, one argmax for the deficit), the u16
//                      tables of the stream, the coder's table -- start, 4096 - f
//                      and a reciprocal of f per symbol -- and the header.
//   enc_code_kernel    one lane per segment, last symbol first; the words a
//                      segment emits go to its slots of the workspace, and each
//                      wave of 64 segments leaves the bytes its segments take.
//   enc_place_kernel   a workgroup per 64 segments: the exclusive scan of 4 + 2 *
//                      words (the waves' sums before it, then a scan over its own
//                      64) -> the directory, payload_bytes and the frame's coded
//                      length; then a wave per segment stores the final state and
//                      the staged words in reverse order of emission.
// The frames' splat counts and byte ranges are kernel arguments computed from
// the host's counts; nothing is sized by a header in device memory.
#include <vector>

#include "ans.h"

namespace gsvc {

constexpr int kEncFrames = 32;      // frames per launch
constexpr int kEncHistBlock = 256;
constexpr int kEncHistSplats = kEncHistBlock * 8;  // splats per workgroup of the histogram kernel
constexpr int kEncTablesBlock = 64 * kAnsChannels;  // a wave per channel
constexpr int kEncCodeBlock = 64;   // one wave: 5 KiB of LDS, so the segments spread over the CUs
constexpr int kEncChunk = 4;        // splats per set of plane loads
constexpr int kEncPlaceBlock = 1024;  // sixteen waves: four of a group's 64 segments each

struct EncodeArgs {
    int nframes, segment;
    long long n[kEncFrames];          // splats, from the host
    long long in_off[kEncFrames];     // the version-1 frame: 256 + 7 n bytes from here
    long long out_off[kEncFrames];    // the frame's slot of the output
    long long hist_off[kEncFrames];   // workspace: u32 [hist_blocks(n)][656] partial histograms
    long long seg_off[kEncFrames];    // workspace: u32 words[n_seg], state[n_seg], bytes[ceil(n_seg / 64)]
    long long stage_off[kEncFrames];  // workspace: u16 [7 n], segment k's words from 7 k S
};

__host__ __device__ inline long long enc_hist_blocks(long long n) {
    return n > 0 ? (n + kEncHistSplats - 1) / kEncHistSplats : 1;
}

// The coder's table entry of a symbol with frequency f and start b:
//   .x  the low 32 bits of m = ceil(2^(32 + l) / f), l = ceil(log2 f) (2^32 <= m < 2^33)
//   .y  b | (4096 - f) << 12 | max(l - 1, 0) << 24 | (f == 1) << 28
// and zero for a symbol that does not occur.
__device__ __forceinline__ uint2 enc_entry(unsigned f, unsigned b) {
    if (f == 0) return make_uint2(0u, 0u);
    if (f == 1) return make_uint2(0u, b | (unsigned)(kProbOne - 1) << 12 | 1u << 28);
    const unsigned l = 32u - (unsigned)__builtin_clz(f - 1u);
    const unsigned long long m = ((1ull << (32 + l)) + f - 1u) / f;
    return make_uint2((unsigned)m, b | ((unsigned)kProbOne - f) << 12 | (l - 1u) << 24);
}

// One symbol: `out` says whether the 16-bit word `word` leaves first.
// x / f = (m x) >> (32 + l) exactly for every x < 2^32; with
// q = x / f the new state ((q << 12) + x % f + b) is x + b + q (4096 - f).
__device__ __forceinline__ unsigned enc_step(unsigned x, uint2 e, bool &out, unsigned &word) {
    const unsigned b = e.y & 4095u, cf = (e.y >> 12) & 4095u, sh = (e.y >> 24) & 15u;
    // x >= (uint64)f << 20: f << 20 has no low bits, and x >> 20 < 4096 never reaches f = 4096
    out = (x >> 20) >= (unsigned)kProbOne - cf;
    word = x & 0xffffu;
    x = out ? x >> 16 : x;
    const unsigned t = __umulhi(x, e.x);
    unsigned q = (t + ((x - t) >> 1)) >> sh;
    q = (e.y >> 28) ? x : q;
    return x + b + __umul24(q, cf);  // q < 2^20, 4096 - f < 2^12
}

__device__ __forceinline__ void st_u16(unsigned char *p, unsigned v) {
    if ((reinterpret_cast<uintptr_t>(p) & 1) == 0) {
        *reinterpret_cast<unsigned short *>(p) = (unsigned short)v;
    } else {
        p[0] = (unsigned char)v;
        p[1] = (unsigned char)(v >> 8);
    }
}
__device__ __forceinline__ void st_u32(unsigned char *p, unsigned v) {
    if ((reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        *reinterpret_cast<unsigned *>(p) = v;
    } else {
        st_u16(p, v & 0xffffu);
        st_u16(p + 2, v >> 16);
    }
}

// kDwords dwords from any byte address, bytes outside [lo, hi) read as 0
template <int kDwords>
__device__ __forceinline__ void ld_bytes(uintptr_t addr, uintptr_t lo, uintptr_t hi, unsigned (&v)[kDwords]) {
    const uintptr_t q = addr & ~(uintptr_t)3;
    const unsigned shift = (unsigned)(addr & 3);
    unsigned w[kDwords + 1];
#pragma unroll
    for (int e = 0; e <= kDwords; ++e) w[e] = ld_dword(q + 4 * e, lo, hi);
#pragma unroll
    for (int e = 0; e < kDwords; ++e) v[e] = __builtin_amdgcn_alignbyte(w[e + 1], w[e], shift);
}

// ans._symbols: the seven symbols of a splat from its plane-A dword and its 24
// plane-B bits, each masked to its alphabet
__device__ __forceinline__ void splat_symbols(unsigned a, unsigned w, unsigned (&sym)[kAnsChannels]) {
    sym[0] = w & 63u, sym[1] = (w >> 6) & 63u, sym[2] = (w >> 12) & 63u;
    sym[3] = (w >> 18) & 7u, sym[4] = (w >> 21) & 7u;
    sym[5] = (a >> 8) & 255u, sym[6] = (a >> 24) & 255u;
}

__global__ __launch_bounds__(kEncHistBlock) void enc_hist_kernel(EncodeArgs a,
                                                                 const unsigned char *__restrict__ in,
                                                                 unsigned char *__restrict__ out,
                                                                 unsigned char *__restrict__ ws) {
    __shared__ unsigned hist[kAnsSymbols];
    const int fr = blockIdx.y;
    const long long n = a.n[fr];
    if (blockIdx.x >= enc_hist_blocks(n)) return;  // the grid is the largest frame's
    const unsigned char *pa = in + a.in_off[fr] + kHeaderBytes, *pb = pa + 4 * n;
    unsigned char *low = out + a.out_off[fr] + kCodedFixedBytes;
    for (int i = threadIdx.x; i < kAnsSymbols; i += kEncHistBlock) hist[i] = 0u;
    __syncthreads();
    const bool aligned = (reinterpret_cast<uintptr_t>(pa) & 3) == 0;
    const long long first = (long long)blockIdx.x * kEncHistSplats, end = min(first + kEncHistSplats, n);
    for (long long i = first + threadIdx.x; i < end; i += kEncHistBlock) {
        const unsigned va = aligned ? *reinterpret_cast<const unsigned *>(pa + 4 * i) : rd_u32(pa + 4 * i);
        const unsigned char *q = pb + 3 * i;
        const unsigned vb = (unsigned)q[0] | (unsigned)q[1] << 8 | (unsigned)q[2] << 16;
        unsigned sym[kAnsChannels];
        splat_symbols(va, vb, sym);
#pragma unroll
        for (int c = 0; c < kAnsChannels; ++c) atomicAdd(&hist[ans_first(c) + sym[c]], 1u);
        st_u16(low + 2 * i, (va & 0xffu) | ((va >> 16) & 0xffu) << 8);
    }
    __syncthreads();
    unsigned *part = reinterpret_cast<unsigned *>(ws + a.hist_off[fr]) + (long long)blockIdx.x * kAnsSymbols;
    for (int i = threadIdx.x; i < kAnsSymbols; i += kEncHistBlock) part[i] = hist[i];
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = max(v, (unsigned)__shfl_xor(v, d, 64));
    return v;
}

__global__ __launch_bounds__(kEncTablesBlock) void enc_tables_kernel(EncodeArgs a,
                                                                     const unsigned char *__restrict__ in,
                                                                     unsigned char *__restrict__ out,
                                                                     const unsigned char *__restrict__ ws,
                                                                     uint2 *__restrict__ tabs) {
    __shared__ unsigned counts[kAnsSymbols];
    const int fr = blockIdx.x;
    const long long n = a.n[fr];
    const unsigned *parts = reinterpret_cast<const unsigned *>(ws + a.hist_off[fr]);
    const long long nparts = enc_hist_blocks(n);
    const unsigned n_seg = (unsigned)((n + a.segment - 1) / a.segment);
    const unsigned char *src = in + a.in_off[fr];
    unsigned char *dst = out + a.out_off[fr];
    // bytes 0-239 of the version-1 header with version = 2 and the host's N, then
    // S, prob_bits, n_seg and the reserved zero; payload_bytes is the place kernel's to write
    for (int i = threadIdx.x; i < kHeaderBytes; i += kEncTablesBlock) {
        unsigned char v = i < kOffSegment ? src[i] : 0;
        if (i >= kOffVersion && i < kOffVersion + 4) v = i == kOffVersion ? GSVC_STREAM_VERSION_CODED : 0;
        if (i >= kOffN && i < kOffN + 4) v = (unsigned char)((unsigned)n >> (8 * (i - kOffN)));
        if (i >= kOffSegment && i < kOffSegment + 2) v = (unsigned char)((unsigned)a.segment >> (8 * (i - kOffSegment)));
        if (i == kOffProbBits) v = kProbBits;
        if (i >= kOffNumSeg && i < kOffNumSeg + 4) v = (unsigned char)(n_seg >> (8 * (i - kOffNumSeg)));
        if (i < kOffPayload || i >= kOffReserved) dst[i] = v;
    }
    // the workgroups' counts of every symbol, summed in block order (a count is at most n < 2^31)
    for (int s = threadIdx.x; s < kAnsSymbols; s += kEncTablesBlock) {
        unsigned cnt = 0u;
        long long p = 0;
        for (; p + 8 <= nparts; p += 8) {  // eight loads in flight
            unsigned v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = parts[(p + j) * kAnsSymbols + s];
#pragma unroll
            for (int j = 0; j < 8; ++j) cnt += v[j];
        }
        for (; p < nparts; ++p) cnt += parts[p * kAnsSymbols + s];
        counts[s] = cnt;
    }
    __syncthreads();
    // A wave per channel; lane l holds the symbols l * per ... l * per + per - 1.
    const int lane = threadIdx.x & 63, c = threadIdx.x >> 6;
    static_assert(kEncTablesBlock == 64 * kAnsChannels, "a wave per channel");
    {
        const int A = ans_alphabet(c), per = A >= 64 ? A / 64 : 1, owners = A / per;
        const bool owner = lane < owners;
        unsigned f[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < per && owner) {
                const unsigned cnt = min(counts[ans_first(c) + lane * per + i], (unsigned)n);
                // floor(4096 cnt / n) by long division: twelve quotient bits, the
                // remainder below n < 2^31 (the product itself would need 43 bits)
                unsigned q = 0u, r = cnt < (unsigned)n ? cnt : 0u;
#pragma unroll
                for (int bit = 0; bit < kProbBits; ++bit) {
                    r <<= 1, q <<= 1;
                    if (r >= (unsigned)n) r -= (unsigned)n, ++q;
                }
                f[i] = cnt ? max(cnt < (unsigned)n ? q : (unsigned)kProbOne, 1u) : 0u;
            }
        unsigned sum = wave_sum(f[0] + f[1] + f[2] + f[3]);
        if (sum == 0u) {  // N = 0
            if (lane == 0) f[0] = kProbOne;
            sum = kProbOne;
        }
        // the largest frequency, the lowest symbol on ties: the largest f << 8 | 255 - symbol
        auto largest = [&]() {
            unsigned key = 0u;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < per && owner) key = max(key, f[i] << 8 | (unsigned)(255 - (lane * per + i)));
            return wave_max(key);
        };
        if (sum > (unsigned)kProbOne) {
            // "While the sum exceeds 4096 the largest loses one, the lowest symbol on
            // ties", E = sum - 4096 < alphabet times, all at once: the loop lowers
            // whatever stands above a level before it touches the level, so with T
            // the largest level at which sum max(0, f - T) >= E, every f above T + 1
            // comes down to T + 1, and the R = E - sum max(0, f - (T + 1)) units left
            // (0 < R <= the symbols now at T + 1) go to the R lowest symbols at T + 1.
            const unsigned E = sum - (unsigned)kProbOne, M = largest() >> 8;
            auto above = [&](unsigned level) {
                unsigned d = 0u;
#pragma unroll
                for (int i = 0; i < 4; ++i) d += f[i] > level ? f[i] - level : 0u;
                return wave_sum(d);
            };
            // above(lo) >= E (the largest alone stands E above M - E), above(hi) = 0 < E
            unsigned lo = M > E ? M - E : 0u, hi = M;
            while (hi - lo > 1u) {
                const unsigned mid = (lo + hi) >> 1;
                if (above(mid) >= E) lo = mid; else hi = mid;
            }
            const unsigned top = lo + 1u, R = E - above(top);
            unsigned at_top = 0u;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f[i] = min(f[i], top);
                at_top += f[i] == top;
            }
            unsigned rank = at_top;  // symbols at the top level in the lanes before this one
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned v = __shfl_up(rank, d, 64);
                if (lane >= d) rank += v;
            }
            rank -= at_top;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (f[i] == top && rank++ < R) --f[i];
        } else if (sum < (unsigned)kProbOne) {
            const unsigned key = largest();
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < per && owner && (f[i] << 8 | (unsigned)(255 - (lane * per + i))) == key)
                    f[i] += (unsigned)kProbOne - sum;
        }
        // starts: an exclusive scan over the lanes, then along the lane's symbols
        const unsigned mine = f[0] + f[1] + f[2] + f[3];
        unsigned incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        unsigned run = incl - mine;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < per && owner) {
                const int s = ans_first(c) + lane * per + i;
                st_u16(dst + kHeaderBytes + 2 * s, f[i]);
                tabs[(long long)fr * kAnsSymbols + s] = enc_entry(f[i], run);
                run += f[i];
            }
    }
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(kEncCodeBlock) void enc_code_kernel(EncodeArgs a,
                                                                 const unsigned char *__restrict__ in,
                                                                 const uint2 *__restrict__ tabs,
                                                                 unsigned char *__restrict__ ws) {
    __shared__ uint2 tab[kAnsSymbols];
    const int fr = blockIdx.y;
    const long long n = a.n[fr];
    const int S = a.segment;
    const long long n_seg = (n + S - 1) / S;
    if ((long long)blockIdx.x * kEncCodeBlock >= n_seg) return;  // the grid is the largest frame's
    for (int i = threadIdx.x; i < kAnsSymbols; i += kEncCodeBlock) tab[i] = tabs[(long long)fr * kAnsSymbols + i];
    __syncthreads();
    const long long k = (long long)blockIdx.x * kEncCodeBlock + threadIdx.x;
    unsigned *seg = reinterpret_cast<unsigned *>(ws + a.seg_off[fr]);
    unsigned bytes = 0u;
    if (k < n_seg) {
        // every plane read is checked against [lo, hi), the frame's 7 n plane bytes
        const uintptr_t lo = reinterpret_cast<uintptr_t>(in + a.in_off[fr] + kHeaderBytes);
        const uintptr_t hi = lo + (uintptr_t)(kSplatBytes * n), pb = lo + (uintptr_t)(4 * n);
        const long long i0 = k * S, i1 = min(i0 + S, n);
        // segment k emits at most one word per symbol: slots [7 i0, 7 i1) of the frame's 7 n
        unsigned short *words = reinterpret_cast<unsigned short *>(ws + a.stage_off[fr]) + kAnsChannels * i0;
        unsigned x = kRansL, cnt = 0u;
        long long c0 = i0 + (i1 - i0 - 1) / kEncChunk * kEncChunk;  // the last chunk, whole or not
        unsigned va[kEncChunk], vb[3];
        static_assert(kEncChunk == 4, "three dwords of plane B per chunk");
        ld_bytes(lo + (uintptr_t)(4 * c0), lo, hi, va);
        ld_bytes(pb + (uintptr_t)(3 * c0), lo, hi, vb);
        for (; c0 >= i0; c0 -= kEncChunk) {
            // the chunk before this one is loaded ahead of this one's chain
            unsigned na[kEncChunk] = {0u, 0u, 0u, 0u}, nb[3] = {0u, 0u, 0u};
            if (c0 - kEncChunk >= i0) {
                ld_bytes(lo + (uintptr_t)(4 * (c0 - kEncChunk)), lo, hi, na);
                ld_bytes(pb + (uintptr_t)(3 * (c0 - kEncChunk)), lo, hi, nb);
            }
            const int have = (int)min((long long)kEncChunk, i1 - c0);
            const unsigned w24[kEncChunk] = {vb[0] & 0xffffffu, vb[0] >> 24 | (vb[1] & 0xffffu) << 8,
                                             vb[1] >> 16 | (vb[2] & 0xffu) << 16, vb[2] >> 8};
#pragma unroll
            for (int t = kEncChunk - 1; t >= 0; --t)
                if (t < have) {
                    unsigned sym[kAnsChannels];
                    splat_symbols(va[t], w24[t], sym);
#pragma unroll
                    for (int c = kAnsChannels - 1; c >= 0; --c) {
                        bool emit;
                        unsigned word;
                        x = enc_step(x, tab[ans_first(c) + sym[c]], emit, word);
                        if (emit) words[cnt++] = (unsigned short)word;
                    }
                }
#pragma unroll
            for (int e = 0; e < kEncChunk; ++e) va[e] = na[e];
#pragma unroll
            for (int e = 0; e < 3; ++e) vb[e] = nb[e];
        }
        seg[k] = cnt;
        seg[n_seg + k] = x;
        bytes = 4u + 2u * cnt;
    }
    // what this wave's segments take in the payload (at most 64 (4 + 14 S) bytes)
    const unsigned long long total = wave_sum64(bytes);
    if (threadIdx.x == 0) seg[2 * n_seg + blockIdx.x] = (unsigned)total;
}

// One workgroup per kEncCodeBlock segments, the code kernel's waves.  Every
// count read back from the workspace is held to what its slots were sized for
// -- a segment's words to one per symbol, a wave's bytes to 4 per segment and
// 14 per splat -- so every offset stays inside the frame's worst-case payload
// whatever the workspace holds.
__global__ __launch_bounds__(kEncPlaceBlock) void enc_place_kernel(EncodeArgs a,
                                                                   unsigned char *__restrict__ out,
                                                                   const unsigned char *__restrict__ ws,
                                                                   long long *__restrict__ coded_bytes) {
    static_assert(kEncCodeBlock == 64, "a wave scans the 64 segments of a code-kernel wave");
    const int fr = blockIdx.y;
    const long long n = a.n[fr];
    const int S = a.segment;
    const long long n_seg = (n + S - 1) / S;
    const long long g = blockIdx.x, first = g * kEncCodeBlock;
    unsigned char *dst = out + a.out_off[fr];
    unsigned char *dir = dst + kCodedFixedBytes + 2 * n;
    const long long fixed = kCodedFixedBytes + 2 * n + 4 * (n_seg + 1);
    if (first >= n_seg) {
        if (n_seg == 0 && g == 0 && threadIdx.x == 0) {  // the empty frame: a directory of one zero
            st_u32(dir, 0u);
            st_u32(dst + kOffPayload, 0u);
            coded_bytes[fr] = fixed;
        }
        return;
    }
    const unsigned *seg = reinterpret_cast<const unsigned *>(ws + a.seg_off[fr]);
    const unsigned short *stage = reinterpret_cast<const unsigned short *>(ws + a.stage_off[fr]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // every wave: the bytes of the waves before this one, then a scan over its own segments
    unsigned long long before = 0;
    for (long long b = lane; b < g; b += 64) {
        const long long s0 = b * kEncCodeBlock * S;  // wave b's splats and segments, all whole
        before += min((unsigned long long)seg[2 * n_seg + b],
                      4ull * kEncCodeBlock + 2ull * kAnsChannels * (unsigned long long)(min(s0 + (long long)kEncCodeBlock * S, n) - s0));
    }
    before = wave_sum64(before);
    const long long k = first + lane;
    const long long i0 = min(k * S, n), i1 = min(i0 + S, n);
    const unsigned cnt = k < n_seg ? min(seg[k], (unsigned)(kAnsChannels * (i1 - i0))) : 0u;
    const unsigned x = k < n_seg ? seg[n_seg + k] : 0u;
    const unsigned mine = k < n_seg ? 4u + 2u * cnt : 0u;
    unsigned incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned v = __shfl_up(incl, d, 64);
        if (lane >= d) incl += v;
    }
    const unsigned d0 = (unsigned)before + incl - mine;  // below 2^32: the host refused a larger worst case
    if (wave == 0 && k < n_seg) {
        st_u32(dir + 4 * k, d0);
        if (k == n_seg - 1) {
            st_u32(dir + 4 * n_seg, d0 + mine);
            st_u32(dst + kOffPayload, d0 + mine);
            coded_bytes[fr] = fixed + (long long)(d0 + mine);
        }
    }
    unsigned char *pay = dst + fixed;
    for (int j = wave; j < kEncCodeBlock && first + j < n_seg; j += kEncPlaceBlock / 64) {
        const unsigned cj = __shfl(cnt, j, 64), xj = __shfl(x, j, 64);
        unsigned char *p = pay + __shfl(d0, j, 64);
        if (lane == 0) st_u32(p, xj);
        const unsigned short *words = stage + kAnsChannels * (first + j) * S;
        for (unsigned w = lane; w < cj; w += 64) st_u16(p + 4 + 2 * w, words[cj - 1 - w]);
    }
}

// Where the frames and the encoder's intermediates lie, from the host's counts.
struct EncodePlan {
    std::vector<long long> in_off, out_off;               // num_frames + 1 each
    std::vector<long long> hist_off, seg_off, stage_off;  // per frame, bytes into the workspace
    long long tabs_off = 0, workspace = 0;
};

static long long round_up(long long v, long long to) { return (v + to - 1) / to * to; }

static int plan_encode(const char *who, int num_frames, const int *num_points, int segment,
                       EncodePlan &p) {
    if (num_frames < 0) return set_error(GSVC_ERR_ARG, "%s: num_frames < 0", who);
    if (num_frames > 0 && !num_points) return set_error(GSVC_ERR_ARG, "%s: null num_points", who);
    if (segment < 1 || segment > kMaxSegment)
        return set_error(GSVC_ERR_ARG, "%s: segment = %d, not in 1..%d", who, segment, kMaxSegment);
    p.in_off.assign(1, 0);
    p.out_off.assign(1, 0);
    p.tabs_off = 0;
    long long at = (long long)num_frames * kAnsSymbols * (long long)sizeof(uint2);
    for (int f = 0; f < num_frames; ++f) {
        const long long n = num_points[f];
        if (n < 0) return set_error(GSVC_ERR_ARG, "%s: frame %d has %lld splats", who, f, n);
        const long long n_seg = (n + segment - 1) / segment;
        // every symbol emits a word: what the directory's u32 offsets must hold
        const long long payload = 4 * n_seg + 2 * kAnsChannels * n;
        if (payload > 0xffffffffll)
            return set_error(GSVC_ERR_ARG, "%s: frame %d: a payload of up to %lld bytes does not fit the "
                                           "stream's u32 offsets", who, f, payload);
        p.in_off.push_back(p.in_off.back() + kHeaderBytes + kSplatBytes * n);
        p.out_off.push_back(p.out_off.back() +
                            round_up(kCodedFixedBytes + 2 * n + 4 * (n_seg + 1) + payload, 4));
        at = round_up(at, 16);
        p.hist_off.push_back(at);
        at = round_up(at + enc_hist_blocks(n) * kAnsSymbols * 4, 16);
        p.seg_off.push_back(at);
        at = round_up(at + 4 * (2 * n_seg + (n_seg + kEncCodeBlock - 1) / kEncCodeBlock), 16);
        p.stage_off.push_back(at);
        at += 2 * kAnsChannels * n;
    }
    p.workspace = round_up(at, 16);
    return GSVC_OK;
}

}  // namespace gsvc

using namespace gsvc;

extern "C" int gsvc_encode_stream_bytes(int num_frames, const int *num_points, int segment,
                                        long long *coded_offsets, size_t *workspace_bytes) {
    EncodePlan p;
    int rc = plan_encode("encode_stream_bytes", num_frames, num_points, segment, p);
    if (rc) return rc;
    if (!coded_offsets || !workspace_bytes)
        return set_error(GSVC_ERR_ARG, "encode_stream_bytes: null coded_offsets / workspace_bytes");
    for (int f = 0; f <= num_frames; ++f) coded_offsets[f] = p.out_off[f];
    *workspace_bytes = (size_t)p.workspace;
    return GSVC_OK;
}

extern "C" int gsvc_encode_stream(int num_frames, const int *num_points,
                                  const unsigned char *frames_dev, int segment,
                                  unsigned char *coded_dev, size_t coded_capacity,
                                  long long *coded_bytes_dev, void *workspace, size_t workspace_bytes,
                                  void *stream) {
    EncodePlan p;
    int rc = plan_encode("encode_stream", num_frames, num_points, segment, p);
    if (rc) return rc;
    if (num_frames == 0) return GSVC_OK;
    if ((unsigned long long)p.out_off.back() > (unsigned long long)coded_capacity)
        return set_error(GSVC_ERR_WORKSPACE, "encode_stream: the coded frames may take %lld bytes, the "
                                             "output holds %zu", p.out_off.back(), coded_capacity);
    if ((unsigned long long)p.workspace > (unsigned long long)workspace_bytes)
        return set_error(GSVC_ERR_WORKSPACE, "encode_stream: the workspace needs %lld bytes, it holds %zu",
                         p.workspace, workspace_bytes);
    if (!frames_dev || !coded_dev || !coded_bytes_dev || !workspace)
        return set_error(GSVC_ERR_ARG, "encode_stream: null tensor");
    if (reinterpret_cast<uintptr_t>(workspace) & 15)
        return set_error(GSVC_ERR_ARG, "encode_stream: the workspace is not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    unsigned char *ws = (unsigned char *)workspace;
    for (int f0 = 0; f0 < num_frames; f0 += kEncFrames) {
        EncodeArgs a;
        a.nframes = std::min(kEncFrames, num_frames - f0);
        a.segment = segment;
        long long nmax = 0;
        for (int i = 0; i < kEncFrames; ++i) {
            const int f = std::min(f0 + i, num_frames - 1);
            a.n[i] = num_points[f];
            a.in_off[i] = p.in_off[f];
            a.out_off[i] = p.out_off[f];
            a.hist_off[i] = p.hist_off[f];
            a.seg_off[i] = p.seg_off[f];
            a.stage_off[i] = p.stage_off[f];
            if (i < a.nframes) nmax = std::max(nmax, a.n[i]);
        }
        const unsigned y = (unsigned)a.nframes;
        const long long max_seg = (nmax + segment - 1) / segment;
        // one wave of the code kernel and one workgroup of the place kernel per 64 segments
        const unsigned seg_blocks = (unsigned)std::max(1ll, (max_seg + kEncCodeBlock - 1) / kEncCodeBlock);
        uint2 *tabs = reinterpret_cast<uint2 *>(ws + p.tabs_off) + (size_t)f0 * kAnsSymbols;
        hipLaunchKernelGGL(enc_hist_kernel, dim3((unsigned)enc_hist_blocks(nmax), y), dim3(kEncHistBlock), 0, s,
                           a, frames_dev, coded_dev, ws);
        hipLaunchKernelGGL(enc_tables_kernel, dim3(y), dim3(kEncTablesBlock), 0, s, a, frames_dev, coded_dev,
                           ws, tabs);
        hipLaunchKernelGGL(enc_code_kernel, dim3(seg_blocks, y), dim3(kEncCodeBlock), 0, s, a, frames_dev,
                           tabs, ws);
        hipLaunchKernelGGL(enc_place_kernel, dim3(seg_blocks, y), dim3(kEncPlaceBlock), 0, s, a, coded_dev,
                           ws, coded_bytes_dev + f0);
        rc = check_launch("encode_stream");
        if (rc) return rc;
    }
    return GSVC_OK;
}
