// The batch YUV conversions, both directions (gfx950): float RGB planes
// [F, 3, H, W] <-> frames of YUV samples, a whole batch per launch, for every
// colour triple of gsvc_yuv_format (8, 10, 12 or 16 bits; BT.601 or BT.709;
// limited or full range) in six layouts: 4:2:0, 4:2:2 and 4:4:4, each planar
// (planes Y, U, V) or semi-planar (plane Y, then one plane of interleaved U, V
// pairs, U first: NV12 / NV16 / NV24 and the P010 / P210 / P410 families).  Not
// part of the reference, which writes no YUV and reads 8-bit I420 only; that one
// restatement (gsvc_i420_to_rgb, one frame, OpenCV's path) stays in yuv.hip.
//
// One kernel family serves five C entries (DESIGN.md §13d-f tell how three
// generations of it came to be, §13i how they were merged):
//   gsvc_rgb_to_i420                        8-bit planar 4:2:0 out, legacy constants;
//   gsvc_yuv420_to_rgb / gsvc_rgb_to_yuv420 planar 4:2:0 of every other triple;
//   gsvc_yuv_to_rgb / gsvc_rgb_to_yuv       the five other layouts, every triple.
// Each entry refuses what belongs to another (conversion_args), so a format has
// one definition; gsvc_yuv_format_table (host only) is here too.
//
// Arithmetic (include/gsvc_amd.h; integer after the quantizer, so both
// directions are bit-exact against tests/yuv_cases.py, yuv_format_cases.py and
// yuv_layout_cases.py): every channel is clamped to [0, 1] (NaN -> 0), scaled by
// the peak, 0.5 added and truncated; luma at 20 bits per pixel; chroma from the
// SUM of the quantized pixels its sample serves (2x2, 2x1 or 1), shifted by 20 +
// log2 of that count, one rounding.  The coefficients are
// gsvc_yuv_format_table's exact 20-bit ones, evaluated in double on the host,
// but for the legacy triple (8-bit bt601 limited range) OpenCV's three-decimal
// constants (kLegacyTable, as yuv.hip): one definition per colour triple, so
// nv12 is a byte permutation of gsvc_rgb_to_i420's I420.  Every coefficient and
// every sample fits an int; products are widened to 64 bits above 8 bits per
// sample (65535 * 1.2 * 2^20 passes 2^36) and stay int32 at 8 bits (below 1.1e9
// in both directions; tests/test_yuv_out_cpu.py, test_yuv_formats_cpu.py and
// test_yuv_layouts_cpu.py re-derive the bounds).
//
// Semi-planar words above 8 bits carry the value in the high bits (P010: word =
// value << (16 - b)); the shift is applied after loading (low bits ignored) and
// before packing (low bits zero).
//
// Two layouts of the work, same bytes.  Vector (W % 8 == 0 and the buffers
// aligned, vector_path): one lane per R rows x 8 columns (R = 2 at 4:2:0, else
// 1), every load issued before first use; Y moves as 8 samples per row, planar
// chroma as 4 U + 4 V samples (8 + 8 at 4:4:4), interleaved chroma as 8 samples
// per access (two at 4:4:4): 8 samples are 16 bytes at 16 bits and 8 bytes at
// 8 bits, and every such access is aligned to its own width (DESIGN.md §13f
// goes through the layouts).  The float planes must be 16-byte aligned; the
// sample buffers 16-byte too, except in gsvc_rgb_to_i420, whose 8-bit planar
// 4:2:0 accesses are 8 and 4 bytes wide and which has always asked for 8 (an
// 18x24 frame is 648 bytes, so every second frame of a batch starts 8 mod 16).
// Fallback (everything else, odd sizes included; at 4:2:0 with H*W/4 odd the V
// plane and every second frame start at odd or 2-mod-4 offsets): one lane per
// chroma block, sample-wide accesses.  HBM-bound: 12 B read + 1.5 samples
// written per 4:2:0 pixel (+1.5 read with ref).
//
// grid (blocks of one frame, frames), no stride loop: a block lies inside one
// frame.  A frame of more than 2^31 - 1 blocks of 256 chroma blocks is refused
// ("more than one grid of blocks"); gsvc_rgb_to_i420, which used to stride over
// 4096 blocks per frame, inherits that refusal: it needs 2^31 * 256 chroma
// blocks in one frame, which no allocation can hold.
//
// With ref, squared sample differences (one is < 2^32 at 16 bits) are summed in
// 64 bits per lane, then by wave, then by block; one 64-bit atomic add per
// plane and block: exact and run-to-run identical.  Blocks are 256 lanes, but
// 1024 in the vector instances with ref whose lanes hold one row (out_block).
#include <math.h>

#include "common.h"

namespace gsvc {

namespace {

constexpr int kMaxGridY = 65535;  // frames per launch
constexpr int kShift = 20;

struct FmtDev {
    int peak, yoff, coff;
    int cy, crv, cgu, cgv, cbu;
    int yr, yg, yb, ur, ug, ub, vr, vg, vb;
    int msb;  // semi-planar words above 8 bits: value << msb
};

// gsvc_yuv_format_table's 18 integers as the kernels take them
constexpr FmtDev fmt_dev(const long long o[18], int msb) {
    return FmtDev{(int)o[0], (int)o[1], (int)o[2], (int)o[4], (int)o[5], (int)o[6], (int)o[7], (int)o[8],
                  (int)o[9], (int)o[10], (int)o[11], (int)o[12], (int)o[13], (int)o[14], (int)o[15],
                  (int)o[16], (int)o[17], msb};
}

// the legacy triple's constants (OpenCV's three decimals, as yuv.hip), in the
// table's order: what every layout computes with at 8-bit bt601 limited range
constexpr long long kLegacyTable[18] = {255, 16, 128, 1, 1220542, 1673527, -409993, -852492, 2116026,
                                        269484, 528482, 102760, -155188, -305135, 460324, 460324, -385875, -74448};

template <int kBytes>
struct Sample {
    using type = unsigned short;
    using acc = long long;
};
template <>
struct Sample<1> {
    using type = unsigned char;
    using acc = int;
};

// rows and columns of the pixel block one chroma sample serves
template <int kChroma>
struct Block {
    static constexpr int rows = kChroma == 420 ? 2 : 1;
    static constexpr int cols = kChroma == 444 ? 1 : 2;
    static constexpr int shift = kShift + (rows == 2 ? 1 : 0) + (cols == 2 ? 1 : 0);
};

__device__ __forceinline__ int lo16(unsigned w) { return (int)(w & 0xffffu); }
__device__ __forceinline__ int hi16(unsigned w) { return (int)(w >> 16); }
__device__ __forceinline__ int byte_at(unsigned w, int k) { return (int)((w >> (8 * k)) & 255u); }

// Values in [0, 65535] as little-endian words.  The empty asm keeps the clamped
// values opaque: left to itself hipcc folds shift, clamp and the first two
// bytes' packing into gfx950's v_ashr_pk_u8_i32 and ORs bytes 2 and 3 into its
// result as if the upper half of that result were zero; on the MI355X the words
// then came back with bytes 2 and 3 wrong (tests/test_yuv_out_gpu.py caught it,
// DESIGN.md §13d).  pack2 is kept opaque in the same way against the 16-bit
// pack-and-saturate folds.
__device__ __forceinline__ unsigned pack4(int a, int b, int c, int d) {
    asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
    return (unsigned)a | (unsigned)b << 8 | (unsigned)c << 16 | (unsigned)d << 24;
}
__device__ __forceinline__ unsigned pack2(int a, int b) {
    asm volatile("" : "+v"(a), "+v"(b));
    return (unsigned)a | (unsigned)b << 16;
}

template <typename A>
__device__ __forceinline__ int sat(A x, int peak) {
    return x < 0 ? 0 : (x > (A)peak ? peak : (int)x);
}

// n samples (n = 8 or 4, vector layout) at p into v[]
template <int kBytes, int kN>
__device__ __forceinline__ void load_samples(const void *p, int *v) {
    if constexpr (kBytes == 2 && kN == 8) {
        const uint4 w = *reinterpret_cast<const uint4 *>(p);
        v[0] = lo16(w.x), v[1] = hi16(w.x), v[2] = lo16(w.y), v[3] = hi16(w.y);
        v[4] = lo16(w.z), v[5] = hi16(w.z), v[6] = lo16(w.w), v[7] = hi16(w.w);
    } else if constexpr (kBytes == 2 && kN == 4) {
        const uint2 w = *reinterpret_cast<const uint2 *>(p);
        v[0] = lo16(w.x), v[1] = hi16(w.x), v[2] = lo16(w.y), v[3] = hi16(w.y);
    } else if constexpr (kBytes == 1 && kN == 8) {
        const uint2 w = *reinterpret_cast<const uint2 *>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = byte_at(w.x, j), v[4 + j] = byte_at(w.y, j);
    } else {
        const unsigned w = *reinterpret_cast<const unsigned *>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = byte_at(w, j);
    }
}

template <int kBytes, int kN>
__device__ __forceinline__ void store_samples(void *p, const int *v) {
    if constexpr (kBytes == 2 && kN == 8) {
        uint4 w;
        w.x = pack2(v[0], v[1]), w.y = pack2(v[2], v[3]), w.z = pack2(v[4], v[5]), w.w = pack2(v[6], v[7]);
        *reinterpret_cast<uint4 *>(p) = w;
    } else if constexpr (kBytes == 2 && kN == 4) {
        uint2 w;
        w.x = pack2(v[0], v[1]), w.y = pack2(v[2], v[3]);
        *reinterpret_cast<uint2 *>(p) = w;
    } else if constexpr (kBytes == 1 && kN == 8) {
        uint2 w;
        w.x = pack4(v[0], v[1], v[2], v[3]), w.y = pack4(v[4], v[5], v[6], v[7]);
        *reinterpret_cast<uint2 *>(p) = w;
    } else {
        *reinterpret_cast<unsigned *>(p) = pack4(v[0], v[1], v[2], v[3]);
    }
}

// Where one lane's unit lies in a frame (offsets in samples from the frame's
// first).  A unit is kR rows x kCols columns and holds kCC chroma samples of
// each kind on one chroma row.
template <int kChroma, bool kSemi, bool kVec>
struct Unit {
    static constexpr int kR = Block<kChroma>::rows, kBW = Block<kChroma>::cols;
    static constexpr int kCols = kVec ? 8 : kBW, kCC = kCols / kBW;
    size_t plane, cplane, fsize;
    long long units;
    int upr;  // units per row of units

    __device__ __forceinline__ Unit(int h, int w) {
        plane = (size_t)h * w;
        cplane = (size_t)(h / kR) * (w / kBW);
        fsize = plane + 2 * cplane;
        upr = w / kCols;
        units = (long long)(h / kR) * upr;
    }
    // first pixel of the top row; the unit's U sample (planar) or U, V pair (semi)
    __device__ __forceinline__ void at(long long tix, int w, size_t *p0, size_t *c0) const {
        const int i = (int)(tix / upr), k = (int)(tix - (long long)i * upr);
        *p0 = (size_t)(kR * i) * w + (size_t)k * kCols;
        const size_t crow = (size_t)i * (w / kBW) + (size_t)k * kCC;  // in chroma samples of one kind
        *c0 = plane + (kSemi ? 2 * crow : crow);
    }
};

// one unit's samples: ys[kR][kCols], us[kCC], vs[kCC], as values (the P010
// family's shift undone)
template <int kBytes, int kChroma, bool kSemi, bool kVec, int kR, int kCols, int kCC>
__device__ __forceinline__ void load_unit(const typename Sample<kBytes>::type *src, size_t p0, size_t c0,
                                          size_t cplane, int w, int msb, int (*ys)[kCols], int *us, int *vs) {
    if constexpr (kVec) {
#pragma unroll
        for (int r = 0; r < kR; ++r) load_samples<kBytes, 8>(src + p0 + (size_t)r * w, ys[r]);
        if constexpr (kSemi) {
#pragma unroll
            for (int g = 0; g < kCC / 4; ++g) {
                int pair[8];
                load_samples<kBytes, 8>(src + c0 + 8 * g, pair);
#pragma unroll
                for (int j = 0; j < 4; ++j) us[4 * g + j] = pair[2 * j], vs[4 * g + j] = pair[2 * j + 1];
            }
        } else {
            load_samples<kBytes, kCC>(src + c0, us);
            load_samples<kBytes, kCC>(src + c0 + cplane, vs);
        }
    } else {
#pragma unroll
        for (int r = 0; r < kR; ++r)
#pragma unroll
            for (int j = 0; j < kCols; ++j) ys[r][j] = (int)src[p0 + (size_t)r * w + j];
        us[0] = (int)src[c0];
        vs[0] = (int)src[kSemi ? c0 + 1 : c0 + cplane];
    }
    if constexpr (kSemi && kBytes == 2) {
#pragma unroll
        for (int r = 0; r < kR; ++r)
#pragma unroll
            for (int j = 0; j < kCols; ++j) ys[r][j] >>= msb;
#pragma unroll
        for (int j = 0; j < kCC; ++j) us[j] >>= msb, vs[j] >>= msb;
    }
}

// ---------------------------------------------------------------------------
// YUV -> float RGB planes

template <typename A>
__device__ __forceinline__ float chan(A x, int peak, float fpeak) {
    return (float)sat<A>(x >> kShift, peak) / fpeak;
}

template <int kBytes, int kChroma, bool kSemi, bool kVec>
__global__ __launch_bounds__(256) void yuv_to_rgb_kernel(const void *__restrict__ yuv, int h, int w, FmtDev t,
                                                         float *__restrict__ out, int frame0) {
    using S = typename Sample<kBytes>::type;
    using A = typename Sample<kBytes>::acc;
    using U = Unit<kChroma, kSemi, kVec>;
    constexpr int kR = U::kR, kBW = U::kBW, kCols = U::kCols, kCC = U::kCC;
    const U un(h, w);
    const size_t f = (size_t)frame0 + blockIdx.y;
    const S *src = reinterpret_cast<const S *>(yuv) + f * un.fsize;
    float *dst = out + f * 3 * un.plane;
    const long long tix = (long long)blockIdx.x * 256 + threadIdx.x;
    if (tix >= un.units) return;
    size_t p0, c0;
    un.at(tix, w, &p0, &c0);

    int ys[kR][kCols], us[kCC], vs[kCC];
    load_unit<kBytes, kChroma, kSemi, kVec, kR, kCols, kCC>(src, p0, c0, un.cplane, w, t.msb, ys, us, vs);

    const float fpeak = (float)t.peak;
    float o[3][kR][kCols];
#pragma unroll
    for (int j = 0; j < kCC; ++j) {
        const int u = us[j] - t.coff, v = vs[j] - t.coff;
        const A half = (A)1 << (kShift - 1);
        const A ruv = half + (A)t.crv * v;
        const A guv = half + (A)t.cgv * v + (A)t.cgu * u;
        const A buv = half + (A)t.cbu * u;
#pragma unroll
        for (int r = 0; r < kR; ++r)
#pragma unroll
            for (int c = kBW * j; c < kBW * j + kBW; ++c) {
                const A y = (A)max(0, ys[r][c] - t.yoff) * t.cy;
                o[0][r][c] = chan<A>(y + ruv, t.peak, fpeak);
                o[1][r][c] = chan<A>(y + guv, t.peak, fpeak);
                o[2][r][c] = chan<A>(y + buv, t.peak, fpeak);
            }
    }

#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            float *d = dst + c * un.plane + p0 + (size_t)r * w;
            if constexpr (kVec) {
                reinterpret_cast<float4 *>(d)[0] = make_float4(o[c][r][0], o[c][r][1], o[c][r][2], o[c][r][3]);
                reinterpret_cast<float4 *>(d)[1] = make_float4(o[c][r][4], o[c][r][5], o[c][r][6], o[c][r][7]);
            } else {
#pragma unroll
                for (int j = 0; j < kCols; ++j) d[j] = o[c][r][j];
            }
        }
}

// ---------------------------------------------------------------------------
// float RGB planes -> YUV (+ SSE against ref)

__device__ __forceinline__ int quant(float x, float fpeak) {
    const float c = fminf(fmaxf(x, 0.0f), 1.0f);
    return (int)__fadd_rn(__fmul_rn(c, fpeak), 0.5f);
}

__device__ __forceinline__ unsigned long long sqdiff(int a, int b) {
    const int d = a - b;  // |d| <= 65535: d * d < 2^32
    return (unsigned long long)((unsigned)d * (unsigned)d);
}

// Lanes per block of an output instance.  With ref every block ends in three
// 64-bit atomic adds on its frame's sse words, and a batch's words share a cache
// line or two: where a lane holds one row (4:2:2, 4:4:4) a 1080p frame is 1013
// blocks of 256 lanes, twice the 4:2:0 count, and the adds queue up behind one
// another; 1024 lanes per block make them a quarter as many.
template <int kChroma, bool kVec, bool kRef>
constexpr int out_block() {
    return (kRef && kVec && Block<kChroma>::rows == 1) ? 1024 : 256;
}

// kLegacyImm (gsvc_rgb_to_i420's instances): the legacy triple's constants as
// immediates instead of the argument's.  Its instance without ref also asks for
// the registers of 7 waves per SIMD, which yuv_out.hip's kernel had and which
// the vector layout otherwise misses by three VGPRs (75); the one with ref has
// them unasked (72) and measures the same either way.
template <int kBytes, int kChroma, bool kSemi, bool kVec, bool kRef, bool kLegacyImm>
__global__ __launch_bounds__((out_block<kChroma, kVec, kRef>()))
__attribute__((amdgpu_waves_per_eu(kLegacyImm && !kRef ? 7 : 1)))
void rgb_to_yuv_kernel(const float *__restrict__ rgb, int h, int w, FmtDev targ, void *__restrict__ out,
                       const void *__restrict__ ref, unsigned long long *__restrict__ sse, int frame0) {
    constexpr FmtDev kImm = fmt_dev(kLegacyTable, 0);
    const FmtDev t = kLegacyImm ? kImm : targ;
    using S = typename Sample<kBytes>::type;
    using A = typename Sample<kBytes>::acc;
    using U = Unit<kChroma, kSemi, kVec>;
    constexpr int kR = U::kR, kBW = U::kBW, kCols = U::kCols, kCC = U::kCC;
    constexpr int kCShift = Block<kChroma>::shift;
    const U un(h, w);
    const size_t f = (size_t)frame0 + blockIdx.y;
    const float *src = rgb + f * 3 * un.plane;
    S *dst = reinterpret_cast<S *>(out) + f * un.fsize;
    const S *rf = kRef ? reinterpret_cast<const S *>(ref) + f * un.fsize : nullptr;
    constexpr int kBlock = out_block<kChroma, kVec, kRef>(), kWaves = kBlock / 64;
    const long long tix = (long long)blockIdx.x * kBlock + threadIdx.x;
    unsigned long long acc[3] = {0ull, 0ull, 0ull};

    if (tix < un.units) {
        size_t p0, c0;
        un.at(tix, w, &p0, &c0);
        const float fpeak = (float)t.peak;
        int q[3][kR][kCols];
        int ry[kR][kCols], ru[kCC], rv[kCC];
        if constexpr (kVec) {
            float4 v[3][kR][2];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int r = 0; r < kR; ++r) {
                    const float4 *s = reinterpret_cast<const float4 *>(src + c * un.plane + p0 + (size_t)r * w);
                    v[c][r][0] = s[0];
                    v[c][r][1] = s[1];
                }
            if constexpr (kRef)
                load_unit<kBytes, kChroma, kSemi, kVec, kR, kCols, kCC>(rf, p0, c0, un.cplane, w, t.msb, ry, ru, rv);
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int r = 0; r < kR; ++r) {
                    const float4 a = v[c][r][0], b = v[c][r][1];
                    q[c][r][0] = quant(a.x, fpeak);
                    q[c][r][1] = quant(a.y, fpeak);
                    q[c][r][2] = quant(a.z, fpeak);
                    q[c][r][3] = quant(a.w, fpeak);
                    q[c][r][4] = quant(b.x, fpeak);
                    q[c][r][5] = quant(b.y, fpeak);
                    q[c][r][6] = quant(b.z, fpeak);
                    q[c][r][7] = quant(b.w, fpeak);
                }
        } else {
            float v[3][kR][kCols];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int r = 0; r < kR; ++r)
#pragma unroll
                    for (int j = 0; j < kCols; ++j) v[c][r][j] = src[c * un.plane + p0 + (size_t)r * w + j];
            if constexpr (kRef)
                load_unit<kBytes, kChroma, kSemi, kVec, kR, kCols, kCC>(rf, p0, c0, un.cplane, w, t.msb, ry, ru, rv);
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int r = 0; r < kR; ++r)
#pragma unroll
                    for (int j = 0; j < kCols; ++j) q[c][r][j] = quant(v[c][r][j], fpeak);
        }

        const A ybias = ((A)t.yoff << kShift) + ((A)1 << (kShift - 1));
        const A cbias = ((A)t.coff << kCShift) + ((A)1 << (kCShift - 1));
        int y[kR][kCols], us[kCC], vs[kCC];
#pragma unroll
        for (int r = 0; r < kR; ++r)
#pragma unroll
            for (int j = 0; j < kCols; ++j)
                y[r][j] = sat<A>(((A)t.yr * q[0][r][j] + (A)t.yg * q[1][r][j] + (A)t.yb * q[2][r][j] + ybias) >>
                                     kShift, t.peak);
#pragma unroll
        for (int j = 0; j < kCC; ++j) {
            int s[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                s[c] = 0;
#pragma unroll
                for (int r = 0; r < kR; ++r)
#pragma unroll
                    for (int b = 0; b < kBW; ++b) s[c] += q[c][r][kBW * j + b];
            }
            us[j] = sat<A>(((A)t.ur * s[0] + (A)t.ug * s[1] + (A)t.ub * s[2] + cbias) >> kCShift, t.peak);
            vs[j] = sat<A>(((A)t.vr * s[0] + (A)t.vg * s[1] + (A)t.vb * s[2] + cbias) >> kCShift, t.peak);
        }

        // the words: the P010 family's shift before packing
        const int msb = (kSemi && kBytes == 2) ? t.msb : 0;
        if constexpr (kVec) {
#pragma unroll
            for (int r = 0; r < kR; ++r) {
                int wy[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) wy[j] = y[r][j] << msb;
                store_samples<kBytes, 8>(dst + p0 + (size_t)r * w, wy);
            }
            if constexpr (kSemi) {
#pragma unroll
                for (int g = 0; g < kCC / 4; ++g) {
                    int pair[8];
#pragma unroll
                    for (int j = 0; j < 4; ++j) pair[2 * j] = us[4 * g + j] << msb, pair[2 * j + 1] = vs[4 * g + j] << msb;
                    store_samples<kBytes, 8>(dst + c0 + 8 * g, pair);
                }
            } else {
                store_samples<kBytes, kCC>(dst + c0, us);
                store_samples<kBytes, kCC>(dst + c0 + un.cplane, vs);
            }
        } else {
#pragma unroll
            for (int r = 0; r < kR; ++r)
#pragma unroll
                for (int j = 0; j < kCols; ++j) dst[p0 + (size_t)r * w + j] = (S)(y[r][j] << msb);
            dst[c0] = (S)(us[0] << msb);
            dst[kSemi ? c0 + 1 : c0 + un.cplane] = (S)(vs[0] << msb);
        }

        if constexpr (kRef) {
#pragma unroll
            for (int r = 0; r < kR; ++r)
#pragma unroll
                for (int j = 0; j < kCols; ++j) acc[0] += sqdiff(y[r][j], ry[r][j]);
#pragma unroll
            for (int j = 0; j < kCC; ++j) acc[1] += sqdiff(us[j], ru[j]), acc[2] += sqdiff(vs[j], rv[j]);
        }
    }

    if constexpr (kRef) {  // every lane arrives: no early exit above
        __shared__ unsigned long long part[kWaves][3];
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc[p] += __shfl_down(acc[p], o);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) {
#pragma unroll
            for (int p = 0; p < 3; ++p) part[wave][p] = acc[p];
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            const int p = threadIdx.x;
            unsigned long long sum = 0ull;  // integers: any order gives the same sum
#pragma unroll
            for (int wv = 0; wv < kWaves; ++wv) sum += part[wv][p];
            atomicAdd(&sse[f * 3 + p], sum);
        }
    }
}

// ---------------------------------------------------------------------------
// host

double fix20(double x) { return floor(x * 1048576.0 + 0.5); }

// nullptr when the format is one of the 16; else what is wrong with it
const char *table_of(const gsvc_yuv_format *fmt, long long o[18]) {
    if (!fmt) return "missing format";
    const int b = fmt->bit_depth;
    if (b != 8 && b != 10 && b != 12 && b != 16) return "bit_depth must be 8, 10, 12 or 16";
    if (fmt->matrix != 0 && fmt->matrix != 1) return "matrix must be 0 (bt601) or 1 (bt709)";
    if (fmt->full_range != 0 && fmt->full_range != 1) return "full_range must be 0 or 1";
    const double kr = fmt->matrix ? 0.2126 : 0.299, kb = fmt->matrix ? 0.0722 : 0.114, kg = 1.0 - kr - kb;
    const long long peak = (1ll << b) - 1;
    const double p = (double)peak;
    const double yspan = fmt->full_range ? p : (double)(219ll << (b - 8));
    const double cspan = fmt->full_range ? p : (double)(224ll << (b - 8));
    o[0] = peak;
    o[1] = fmt->full_range ? 0 : (16ll << (b - 8));
    o[2] = 1ll << (b - 1);
    o[3] = b == 8 ? 1 : 2;
    o[4] = (long long)fix20(p / yspan);
    o[5] = (long long)fix20(2.0 * (1.0 - kr) * p / cspan);
    o[6] = (long long)fix20(-2.0 * kb * (1.0 - kb) / kg * p / cspan);
    o[7] = (long long)fix20(-2.0 * kr * (1.0 - kr) / kg * p / cspan);
    o[8] = (long long)fix20(2.0 * (1.0 - kb) * p / cspan);
    o[9] = (long long)fix20(kr * yspan / p);
    o[10] = (long long)fix20(kg * yspan / p);
    o[11] = (long long)fix20(kb * yspan / p);
    o[12] = (long long)fix20(-kr / (2.0 * (1.0 - kb)) * cspan / p);
    o[13] = (long long)fix20(-kg / (2.0 * (1.0 - kb)) * cspan / p);
    o[14] = (long long)fix20(cspan / (2.0 * p));
    o[15] = (long long)fix20(cspan / (2.0 * p));
    o[16] = (long long)fix20(-kg / (2.0 * (1.0 - kr)) * cspan / p);
    o[17] = (long long)fix20(-kb / (2.0 * (1.0 - kr)) * cspan / p);
    return nullptr;
}

const gsvc_yuv_format kLegacyFormat = {8, 0, 0};

// What an entry serves; the rest it refuses, so every format has one entry.
enum Serves {
    kLegacyI420,  // gsvc_rgb_to_i420: the legacy triple, planar 4:2:0
    kPlanar420,   // gsvc_yuv420_to_rgb / gsvc_rgb_to_yuv420: planar 4:2:0 but the legacy triple
    kLayouts      // gsvc_yuv_to_rgb / gsvc_rgb_to_yuv: every layout but planar 4:2:0
};

// The checks every conversion entry shares, under the entry's name; 0 and *t
// filled, or a status.  a, b: the two buffers that must be there; samples, ref:
// the ones that hold samples.
int conversion_args(const char *what, Serves serves, int frames, int h, int w, const gsvc_yuv_format *fmt,
                    int chroma, int semi, const void *a, const void *b, const void *ref, const void *sse,
                    const void *samples, FmtDev *t) {
    if (chroma != 420 && chroma != 422 && chroma != 444)
        return set_error(GSVC_ERR_ARG, "%s: chroma must be 420, 422 or 444, not %d", what, chroma);
    if (semi != 0 && semi != 1) return set_error(GSVC_ERR_ARG, "%s: semi_planar must be 0 or 1", what);
    long long o[18];
    if (const char *bad = table_of(fmt, o))  // the layouts' entries have always named the table here
        return set_error(GSVC_ERR_ARG, "%s: %s", serves == kLayouts ? "yuv_format_table" : what, bad);
    const bool legacy = fmt->bit_depth == 8 && fmt->matrix == 0 && fmt->full_range == 0;
    if (serves == kLayouts && chroma == 420 && !semi)
        return set_error(GSVC_ERR_ARG, "%s: planar 4:2:0 belongs to gsvc_i420_to_rgb / gsvc_rgb_to_i420 and "
                         "gsvc_yuv420_to_rgb / gsvc_rgb_to_yuv420", what);
    if (serves == kPlanar420 && legacy)
        return set_error(GSVC_ERR_ARG, "%s: 8-bit bt601 limited range is the legacy format of "
                         "gsvc_i420_to_rgb / gsvc_rgb_to_i420", what);
    if (frames <= 0) return set_error(GSVC_ERR_ARG, "%s: frames = %d, must be positive", what, frames);
    if (serves == kLayouts) {
        if (h <= 0 || w <= 0) return set_error(GSVC_ERR_ARG, "%s: height and width must be positive", what);
        if (chroma == 420 && ((h & 1) || (w & 1)))
            return set_error(GSVC_ERR_ARG, "%s: 4:2:0 needs an even height and width", what);
        if (chroma == 422 && (w & 1)) return set_error(GSVC_ERR_ARG, "%s: 4:2:2 needs an even width", what);
    } else if (h <= 0 || w <= 0 || (h & 1) || (w & 1))
        return set_error(GSVC_ERR_ARG, "%s: height and width must be positive and even", what);
    if (!a || !b) return set_error(GSVC_ERR_ARG, "%s: missing buffer", what);
    if (ref && !sse) return set_error(GSVC_ERR_ARG, "%s: ref needs sse", what);
    if (o[3] == 2 && (((uintptr_t)samples | (uintptr_t)ref) & 1u))
        return set_error(GSVC_ERR_ARG, "%s: 16-bit samples at an odd address", what);
    // the fallback layout's blocks of 256 chroma blocks, the most of any instance
    const long long blocks = (long long)(chroma == 420 ? h / 2 : h) * (chroma == 444 ? w : w / 2);
    if ((blocks + 255) / 256 > 2147483647ll)
        return set_error(GSVC_ERR_ARG, "%s: %dx%d is more than one grid of blocks", what, h, w);
    if (legacy)
        for (int k = 0; k < 18; ++k) o[k] = kLegacyTable[k];
    *t = fmt_dev(o, (semi && fmt->bit_depth > 8) ? 16 - fmt->bit_depth : 0);
    return GSVC_OK;
}

template <int kChroma, bool kVec, int kBlock = 256>
dim3 grid_of(int h, int w, int fy) {
    const long long units = (long long)(h / Block<kChroma>::rows) * (w / (kVec ? 8 : Block<kChroma>::cols));
    return dim3((unsigned)((units + kBlock - 1) / kBlock), (unsigned)fy);
}

template <int kBytes, int kChroma, bool kSemi>
void launch_in(bool vec, int frames, const void *yuv, int h, int w, const FmtDev &t, float *out, hipStream_t s) {
    for (int f0 = 0; f0 < frames; f0 += kMaxGridY) {
        const int fy = frames - f0 < kMaxGridY ? frames - f0 : kMaxGridY;
        if (vec) {
            const dim3 grid = grid_of<kChroma, true>(h, w, fy);
            hipLaunchKernelGGL((yuv_to_rgb_kernel<kBytes, kChroma, kSemi, true>), grid, dim3(256), 0, s, yuv, h, w,
                               t, out, f0);
        } else {
            const dim3 grid = grid_of<kChroma, false>(h, w, fy);
            hipLaunchKernelGGL((yuv_to_rgb_kernel<kBytes, kChroma, kSemi, false>), grid, dim3(256), 0, s, yuv, h, w,
                               t, out, f0);
        }
    }
}

template <int kBytes, int kChroma, bool kSemi, bool kVec, bool kLegacyImm>
void launch_out(int frames, const float *rgb, int h, int w, const FmtDev &t, void *out, const void *ref,
                unsigned long long *sse, hipStream_t s) {
    for (int f0 = 0; f0 < frames; f0 += kMaxGridY) {
        const int fy = frames - f0 < kMaxGridY ? frames - f0 : kMaxGridY;
        const dim3 grid = grid_of<kChroma, kVec>(h, w, fy);
        if (ref) {
            constexpr int kBlock = out_block<kChroma, kVec, true>();
            const dim3 rgrid = grid_of<kChroma, kVec, kBlock>(h, w, fy);
            hipLaunchKernelGGL((rgb_to_yuv_kernel<kBytes, kChroma, kSemi, kVec, true, kLegacyImm>), rgrid, dim3(kBlock), 0, s,
                               rgb, h, w, t, out, ref, sse, f0);
        } else
            hipLaunchKernelGGL((rgb_to_yuv_kernel<kBytes, kChroma, kSemi, kVec, false, kLegacyImm>), grid, dim3(256), 0, s, rgb,
                               h, w, t, out, nullptr, nullptr, f0);
    }
}

struct InArgs {
    bool vec;
    int frames;
    const void *yuv;
    int h, w;
    FmtDev t;
    float *out;
    hipStream_t s;
};

struct OutArgs {
    bool vec;
    int frames;
    const float *rgb;
    int h, w;
    FmtDev t;
    void *out;
    const void *ref;
    unsigned long long *sse;
    hipStream_t s;
};

template <int kBytes, int kChroma, bool kSemi>
void run(const InArgs &a) {
    launch_in<kBytes, kChroma, kSemi>(a.vec, a.frames, a.yuv, a.h, a.w, a.t, a.out, a.s);
}

template <int kBytes, int kChroma, bool kSemi, bool kLegacyImm = false>
void run(const OutArgs &a) {
    if (a.vec)
        launch_out<kBytes, kChroma, kSemi, true, kLegacyImm>(a.frames, a.rgb, a.h, a.w, a.t, a.out, a.ref, a.sse, a.s);
    else
        launch_out<kBytes, kChroma, kSemi, false, kLegacyImm>(a.frames, a.rgb, a.h, a.w, a.t, a.out, a.ref, a.sse, a.s);
}

// the six layouts
template <int kBytes, typename Args>
void pick_layout(int chroma, bool semi, const Args &a) {
    if (chroma == 420 && semi) run<kBytes, 420, true>(a);
    else if (chroma == 420) run<kBytes, 420, false>(a);
    else if (chroma == 422 && semi) run<kBytes, 422, true>(a);
    else if (chroma == 422) run<kBytes, 422, false>(a);
    else if (semi) run<kBytes, 444, true>(a);
    else run<kBytes, 444, false>(a);
}

// The vector layout's condition: W % 8 == 0, the float planes 16-byte aligned
// and the sample buffers (ref may be null) clear of sample_mask: 15 everywhere
// but in gsvc_rgb_to_i420, which passes 7 (the header comment says why).
bool vector_path(int w, const float *planes, const void *samples, const void *ref, unsigned sample_mask) {
    return w % 8 == 0 && ((uintptr_t)planes & 15u) == 0 &&
           (((uintptr_t)samples | (uintptr_t)ref) & sample_mask) == 0;
}

int convert_in(const char *what, Serves serves, int frames, const void *yuv, int h, int w,
               const gsvc_yuv_format *fmt, int chroma, int semi, float *out, void *stream) {
    FmtDev t;
    if (const int rc = conversion_args(what, serves, frames, h, w, fmt, chroma, semi, yuv, out, nullptr, nullptr,
                                       yuv, &t))
        return rc;
    const InArgs a{vector_path(w, out, yuv, nullptr, 15u), frames, yuv, h, w, t, out, (hipStream_t)stream};
    if (fmt->bit_depth == 8) pick_layout<1>(chroma, semi != 0, a);
    else pick_layout<2>(chroma, semi != 0, a);
    return check_launch(what);
}

int convert_out(const char *what, Serves serves, unsigned sample_mask, int frames, const float *rgb, int h, int w,
                const gsvc_yuv_format *fmt, int chroma, int semi, void *out, const void *ref,
                unsigned long long *sse, void *stream) {
    FmtDev t;
    if (const int rc = conversion_args(what, serves, frames, h, w, fmt, chroma, semi, rgb, out, ref, sse, out, &t))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    if (ref) {
        const int rc = dev_zero(sse, (size_t)frames * 3 * sizeof(unsigned long long), s);
        if (rc) return rc;
    }
    const OutArgs a{vector_path(w, rgb, out, ref, sample_mask), frames, rgb, h, w, t, out, ref, sse, s};
    if (serves == kLegacyI420) run<1, 420, false, true>(a);  // the table as immediates
    else if (fmt->bit_depth == 8) pick_layout<1>(chroma, semi != 0, a);
    else pick_layout<2>(chroma, semi != 0, a);
    return check_launch(what);
}

}  // namespace

}  // namespace gsvc

using namespace gsvc;

extern "C" int gsvc_yuv_format_table(const gsvc_yuv_format *fmt, long long out[18]) {
    if (!out) return set_error(GSVC_ERR_ARG, "yuv_format_table: missing buffer");
    if (const char *bad = table_of(fmt, out)) return set_error(GSVC_ERR_ARG, "yuv_format_table: %s", bad);
    return GSVC_OK;
}

extern "C" int gsvc_rgb_to_i420(int frames, const float *rgb, int height, int width, unsigned char *out,
                                const unsigned char *ref, unsigned long long *sse, void *stream) {
    return convert_out("rgb_to_i420", kLegacyI420, 7u, frames, rgb, height, width, &kLegacyFormat, 420, 0, out, ref,
                       sse, stream);
}

extern "C" int gsvc_yuv420_to_rgb(int frames, const void *yuv, int height, int width,
                                  const gsvc_yuv_format *fmt, float *out, void *stream) {
    return convert_in("yuv420_to_rgb", kPlanar420, frames, yuv, height, width, fmt, 420, 0, out, stream);
}

extern "C" int gsvc_rgb_to_yuv420(int frames, const float *rgb, int height, int width,
                                  const gsvc_yuv_format *fmt, void *out, const void *ref,
                                  unsigned long long *sse, void *stream) {
    return convert_out("rgb_to_yuv420", kPlanar420, 15u, frames, rgb, height, width, fmt, 420, 0, out, ref, sse,
                       stream);
}

extern "C" int gsvc_yuv_to_rgb(int frames, const void *yuv, int height, int width, const gsvc_yuv_format *fmt,
                               int chroma, int semi_planar, float *out, void *stream) {
    return convert_in("yuv_to_rgb", kLayouts, frames, yuv, height, width, fmt, chroma, semi_planar, out, stream);
}

extern "C" int gsvc_rgb_to_yuv(int frames, const float *rgb, int height, int width, const gsvc_yuv_format *fmt,
                               int chroma, int semi_planar, void *out, const void *ref,
                               unsigned long long *sse, void *stream) {
    return convert_out("rgb_to_yuv", kLayouts, 15u, frames, rgb, height, width, fmt, chroma, semi_planar, out, ref,
                       sse, stream);
}

