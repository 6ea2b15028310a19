// Planar YUV 4:2:0 in and out beyond 8-bit BT.601 limited range (gfx950): 8, 10,
// 12 or 16 bits per sample (16-bit little-endian words above 8), BT.601 or
// BT.709, limited or full range, a whole batch per launch.  Not part of the
// reference.  The legacy format stays with yuv.hip / yuv_out.hip (OpenCV's
// three-decimal constants) and is refused here.
//
// Arithmetic (include/gsvc_amd.h; integer after the quantizer, so both
// directions are bit-exact against tests/yuv_format_cases.py): exact 20-bit
// coefficients from gsvc_yuv_format_table, evaluated in double on the host.
// Every coefficient and every sample fits an int; their products are widened
// to 64 bits above 8 bits per sample (65535 * 1.2 * 2^20 passes 2^36) and stay
// int32 at 8 bits (below 1.1e9 in both directions: tests/test_yuv_formats_cpu.py).
//
// Two layouts, same bytes.  Vector (W % 8 == 0, every buffer 16-byte aligned:
// then every plane and frame starts aligned): one lane per 2 rows x 8 columns,
// every load issued before first use; 16-bit samples move as 16 bytes of Y per
// row and 8 bytes of U and of V, 8-bit ones as 8 and 4.  Fallback (everything
// else): one lane per 2x2 block, sample-wide accesses.  grid (blocks of one
// frame, frames), no stride loop: a block lies inside one frame.
//
// With ref, squared sample differences (one is < 2^32 at 16 bits) are summed in
// 64 bits per lane, then by wave, then by block; one 64-bit atomic add per
// plane and block: exact and run-to-run identical.
#include <math.h>

#include "common.h"

namespace gsvc {

namespace {

constexpr int kMaxGridY = 65535;  // frames per launch
constexpr int kShift = 20, kCShift = 22;

struct FmtDev {
    int peak, yoff, coff;
    int cy, crv, cgu, cgv, cbu;
    int yr, yg, yb, ur, ug, ub, vr, vg, vb;
};

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

__device__ __forceinline__ int lo16(unsigned w) { return (int)(w & 0xffffu); }
__device__ __forceinline__ int hi16(unsigned w) { return (int)(w >> 16); }
__device__ __forceinline__ int byte_at(unsigned w, int k) { return (int)((w >> (8 * k)) & 255u); }

// Values in [0, P] as little-endian words.  The empty asm keeps the clamped
// values opaque to the compiler's pack-and-saturate folds (yuv_out.hip pack4,
// DESIGN.md §13d).
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

// ---------------------------------------------------------------------------
// YUV -> float RGB planes

template <typename A>
__device__ __forceinline__ float chan(A x, int peak, float fpeak) {
    return (float)sat<A>(x >> kShift, peak) / fpeak;
}

template <int kBytes, bool kVec>
__global__ __launch_bounds__(256) void yuv420_to_rgb_kernel(const void *__restrict__ yuv, int h, int w,
                                                            FmtDev t, float *__restrict__ out, int frame0) {
    using S = typename Sample<kBytes>::type;
    using A = typename Sample<kBytes>::acc;
    constexpr int kCols = kVec ? 8 : 2;
    const size_t f = (size_t)frame0 + blockIdx.y;
    const size_t plane = (size_t)h * w, cplane = plane / 4, fsize = plane + 2 * cplane;  // samples
    const S *src = reinterpret_cast<const S *>(yuv) + f * fsize;
    float *dst = out + f * 3 * plane;
    const int hw = w / 2, upr = w / kCols;  // units per row pair
    const long long units = (long long)(h / 2) * upr;
    const long long tix = (long long)blockIdx.x * 256 + threadIdx.x;
    if (tix >= units) return;
    const int i2 = (int)(tix / upr), k = (int)(tix - (long long)i2 * upr);
    const size_t p0 = (size_t)(2 * i2) * w + (size_t)k * kCols;                   // top row's first pixel
    const size_t c0 = plane + (size_t)i2 * hw + (size_t)k * (kCols / 2);          // its U sample

    int ys[2][kCols], us[kCols / 2], vs[kCols / 2];
    if constexpr (kVec) {
        load_samples<kBytes, 8>(src + p0, ys[0]);
        load_samples<kBytes, 8>(src + p0 + w, ys[1]);
        load_samples<kBytes, 4>(src + c0, us);
        load_samples<kBytes, 4>(src + c0 + cplane, vs);
    } else {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < 2; ++j) ys[r][j] = (int)src[p0 + (size_t)r * w + j];
        us[0] = (int)src[c0];
        vs[0] = (int)src[c0 + cplane];
    }

    const float fpeak = (float)t.peak;
    float o[3][2][kCols];
#pragma unroll
    for (int j = 0; j < kCols / 2; ++j) {
        const int u = us[j] - t.coff, v = vs[j] - t.coff;
        const A half = (A)1 << (kShift - 1);
        const A ruv = half + (A)t.crv * v;
        const A guv = half + (A)t.cgv * v + (A)t.cgu * u;
        const A buv = half + (A)t.cbu * u;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 2 * j; c < 2 * j + 2; ++c) {
                const A y = (A)max(0, ys[r][c] - t.yoff) * t.cy;
                o[0][r][c] = chan<A>(y + ruv, t.peak, fpeak);
                o[1][r][c] = chan<A>(y + guv, t.peak, fpeak);
                o[2][r][c] = chan<A>(y + buv, t.peak, fpeak);
            }
    }

#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            float *d = dst + c * plane + p0 + (size_t)r * w;
            if constexpr (kVec) {
                reinterpret_cast<float4 *>(d)[0] = make_float4(o[c][r][0], o[c][r][1], o[c][r][2], o[c][r][3]);
                reinterpret_cast<float4 *>(d)[1] = make_float4(o[c][r][4], o[c][r][5], o[c][r][6], o[c][r][7]);
            } else {
                d[0] = o[c][r][0];
                d[1] = o[c][r][1];
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

template <int kBytes, bool kVec, bool kRef>
__global__ __launch_bounds__(256) void rgb_to_yuv420_kernel(const float *__restrict__ rgb, int h, int w,
                                                            FmtDev t, void *__restrict__ out,
                                                            const void *__restrict__ ref,
                                                            unsigned long long *__restrict__ sse, int frame0) {
    using S = typename Sample<kBytes>::type;
    using A = typename Sample<kBytes>::acc;
    constexpr int kCols = kVec ? 8 : 2;
    const size_t f = (size_t)frame0 + blockIdx.y;
    const size_t plane = (size_t)h * w, cplane = plane / 4, fsize = plane + 2 * cplane;  // samples
    const float *src = rgb + f * 3 * plane;
    S *dst = reinterpret_cast<S *>(out) + f * fsize;
    const S *rf = kRef ? reinterpret_cast<const S *>(ref) + f * fsize : nullptr;
    const int hw = w / 2, upr = w / kCols;  // units per row pair
    const long long units = (long long)(h / 2) * upr;
    const long long tix = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long acc[3] = {0ull, 0ull, 0ull};

    if (tix < units) {
        const int i2 = (int)(tix / upr), k = (int)(tix - (long long)i2 * upr);
        const size_t p0 = (size_t)(2 * i2) * w + (size_t)k * kCols;           // top row's first pixel
        const size_t c0 = plane + (size_t)i2 * hw + (size_t)k * (kCols / 2);  // its U sample
        const float fpeak = (float)t.peak;
        int q[3][2][kCols];
        int ry[2][kCols], rc[2][kCols / 2];
        if constexpr (kVec) {
            float4 v[3][2][2];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const float4 *s = reinterpret_cast<const float4 *>(src + c * plane + p0 + (size_t)r * w);
                    v[c][r][0] = s[0];
                    v[c][r][1] = s[1];
                }
            if constexpr (kRef) {
                load_samples<kBytes, 8>(rf + p0, ry[0]);
                load_samples<kBytes, 8>(rf + p0 + w, ry[1]);
                load_samples<kBytes, 4>(rf + c0, rc[0]);
                load_samples<kBytes, 4>(rf + c0 + cplane, rc[1]);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int r = 0; r < 2; ++r) {
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
            float v[3][2][2];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int j = 0; j < 2; ++j) v[c][r][j] = src[c * plane + p0 + (size_t)r * w + j];
            if constexpr (kRef) {
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int j = 0; j < 2; ++j) ry[r][j] = (int)rf[p0 + (size_t)r * w + j];
                rc[0][0] = (int)rf[c0];
                rc[1][0] = (int)rf[c0 + cplane];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int j = 0; j < 2; ++j) q[c][r][j] = quant(v[c][r][j], fpeak);
        }

        const A ybias = ((A)t.yoff << kShift) + ((A)1 << (kShift - 1));
        const A cbias = ((A)t.coff << kCShift) + ((A)1 << (kCShift - 1));
        int y[2][kCols], uv[2][kCols / 2];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < kCols; ++j)
                y[r][j] = sat<A>(((A)t.yr * q[0][r][j] + (A)t.yg * q[1][r][j] + (A)t.yb * q[2][r][j] + ybias) >>
                                     kShift, t.peak);
#pragma unroll
        for (int j = 0; j < kCols / 2; ++j) {
            int s[3];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                s[c] = (q[c][0][2 * j] + q[c][0][2 * j + 1]) + (q[c][1][2 * j] + q[c][1][2 * j + 1]);
            uv[0][j] = sat<A>(((A)t.ur * s[0] + (A)t.ug * s[1] + (A)t.ub * s[2] + cbias) >> kCShift, t.peak);
            uv[1][j] = sat<A>(((A)t.vr * s[0] + (A)t.vg * s[1] + (A)t.vb * s[2] + cbias) >> kCShift, t.peak);
        }

        if constexpr (kVec) {
            store_samples<kBytes, 8>(dst + p0, y[0]);
            store_samples<kBytes, 8>(dst + p0 + w, y[1]);
            store_samples<kBytes, 4>(dst + c0, uv[0]);
            store_samples<kBytes, 4>(dst + c0 + cplane, uv[1]);
        } else {
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int j = 0; j < 2; ++j) dst[p0 + (size_t)r * w + j] = (S)y[r][j];
            dst[c0] = (S)uv[0][0];
            dst[c0 + cplane] = (S)uv[1][0];
        }

        if constexpr (kRef) {
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int j = 0; j < kCols; ++j) acc[0] += sqdiff(y[r][j], ry[r][j]);
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int j = 0; j < kCols / 2; ++j) acc[1 + p] += sqdiff(uv[p][j], rc[p][j]);
        }
    }

    if constexpr (kRef) {  // every lane arrives: no early exit above
        __shared__ unsigned long long part[4][3];
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
            atomicAdd(&sse[f * 3 + p], (part[0][p] + part[1][p]) + (part[2][p] + part[3][p]));
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

// the checks both conversions share; 0 and *t filled, or a status
int conversion_args(const char *what, int frames, int h, int w, const gsvc_yuv_format *fmt, const void *a,
                    const void *b, const void *samples, const void *samples2, FmtDev *t) {
    long long o[18];
    if (const char *bad = table_of(fmt, o)) return set_error(GSVC_ERR_ARG, "%s: %s", what, bad);
    if (fmt->bit_depth == 8 && fmt->matrix == 0 && fmt->full_range == 0)
        return set_error(GSVC_ERR_ARG, "%s: 8-bit bt601 limited range is the legacy format of "
                         "gsvc_i420_to_rgb / gsvc_rgb_to_i420", what);
    if (frames <= 0) return set_error(GSVC_ERR_ARG, "%s: frames = %d, must be positive", what, frames);
    if (h <= 0 || w <= 0 || (h & 1) || (w & 1))
        return set_error(GSVC_ERR_ARG, "%s: height and width must be positive and even", what);
    if (!a || !b) return set_error(GSVC_ERR_ARG, "%s: missing buffer", what);
    if (o[3] == 2 && (((uintptr_t)samples | (uintptr_t)samples2) & 1u))
        return set_error(GSVC_ERR_ARG, "%s: 16-bit samples at an odd address", what);
    if (((long long)(h / 2) * (w / 2) + 255) / 256 > 2147483647ll)
        return set_error(GSVC_ERR_ARG, "%s: %dx%d is more than one grid of blocks", what, h, w);
    *t = FmtDev{(int)o[0], (int)o[1], (int)o[2], (int)o[4], (int)o[5], (int)o[6], (int)o[7], (int)o[8],
                (int)o[9], (int)o[10], (int)o[11], (int)o[12], (int)o[13], (int)o[14], (int)o[15],
                (int)o[16], (int)o[17]};
    return GSVC_OK;
}

dim3 grid_of(int h, int w, bool vec, int fy) {
    const long long units = (long long)(h / 2) * (w / (vec ? 8 : 2));
    return dim3((unsigned)((units + 255) / 256), (unsigned)fy);
}

template <int kBytes, bool kVec>
void launch_in(int frames, const void *yuv, int h, int w, const FmtDev &t, float *out, hipStream_t s) {
    for (int f0 = 0; f0 < frames; f0 += kMaxGridY) {
        const int fy = frames - f0 < kMaxGridY ? frames - f0 : kMaxGridY;
        hipLaunchKernelGGL((yuv420_to_rgb_kernel<kBytes, kVec>), grid_of(h, w, kVec, fy), dim3(256), 0, s, yuv,
                           h, w, t, out, f0);
    }
}

template <int kBytes, bool kVec, bool kRef>
void launch_out(int frames, const float *rgb, int h, int w, const FmtDev &t, void *out, const void *ref,
                unsigned long long *sse, hipStream_t s) {
    for (int f0 = 0; f0 < frames; f0 += kMaxGridY) {
        const int fy = frames - f0 < kMaxGridY ? frames - f0 : kMaxGridY;
        hipLaunchKernelGGL((rgb_to_yuv420_kernel<kBytes, kVec, kRef>), grid_of(h, w, kVec, fy), dim3(256), 0, s,
                           rgb, h, w, t, out, ref, sse, f0);
    }
}

template <int kBytes>
void dispatch_out(bool vec, int frames, const float *rgb, int h, int w, const FmtDev &t, void *out,
                  const void *ref, unsigned long long *sse, hipStream_t s) {
    if (vec) {
        if (ref) launch_out<kBytes, true, true>(frames, rgb, h, w, t, out, ref, sse, s);
        else launch_out<kBytes, true, false>(frames, rgb, h, w, t, out, nullptr, nullptr, s);
    } else {
        if (ref) launch_out<kBytes, false, true>(frames, rgb, h, w, t, out, ref, sse, s);
        else launch_out<kBytes, false, false>(frames, rgb, h, w, t, out, nullptr, nullptr, s);
    }
}

}  // namespace

}  // namespace gsvc

using namespace gsvc;

extern "C" int gsvc_yuv_format_table(const gsvc_yuv_format *fmt, long long out[18]) {
    if (!out) return set_error(GSVC_ERR_ARG, "yuv_format_table: missing buffer");
    if (const char *bad = table_of(fmt, out)) return set_error(GSVC_ERR_ARG, "yuv_format_table: %s", bad);
    return GSVC_OK;
}

extern "C" int gsvc_yuv420_to_rgb(int frames, const void *yuv, int height, int width,
                                  const gsvc_yuv_format *fmt, float *out, void *stream) {
    FmtDev t;
    if (const int rc = conversion_args("yuv420_to_rgb", frames, height, width, fmt, yuv, out, yuv, nullptr, &t))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = (width % 8 == 0) && (((uintptr_t)yuv | (uintptr_t)out) & 15u) == 0;
    if (fmt->bit_depth == 8) {
        if (vec) launch_in<1, true>(frames, yuv, height, width, t, out, s);
        else launch_in<1, false>(frames, yuv, height, width, t, out, s);
    } else {
        if (vec) launch_in<2, true>(frames, yuv, height, width, t, out, s);
        else launch_in<2, false>(frames, yuv, height, width, t, out, s);
    }
    return check_launch("yuv420_to_rgb");
}

extern "C" int gsvc_rgb_to_yuv420(int frames, const float *rgb, int height, int width,
                                  const gsvc_yuv_format *fmt, void *out, const void *ref,
                                  unsigned long long *sse, void *stream) {
    FmtDev t;
    if (const int rc = conversion_args("rgb_to_yuv420", frames, height, width, fmt, rgb, out, out, ref, &t))
        return rc;
    if (ref && !sse) return set_error(GSVC_ERR_ARG, "rgb_to_yuv420: ref needs sse");
    hipStream_t s = (hipStream_t)stream;
    if (ref) {
        const int rc = dev_zero(sse, (size_t)frames * 3 * sizeof(unsigned long long), s);
        if (rc) return rc;
    }
    const uintptr_t at = (uintptr_t)rgb | (uintptr_t)out | (uintptr_t)ref;
    const bool vec = (width % 8 == 0) && (at & 15u) == 0;
    if (fmt->bit_depth == 8) dispatch_out<1>(vec, frames, rgb, height, width, t, out, ref, sse, s);
    else dispatch_out<2>(vec, frames, rgb, height, width, t, out, ref, sse, s);
    return check_launch("rgb_to_yuv420");
}
