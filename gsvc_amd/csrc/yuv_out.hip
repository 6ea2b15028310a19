// Video frame output of the decoder (gfx950): float RGB planes [F, 3, H, W] to
// planar I420 (YUV 4:2:0, 8 bit), a whole batch per launch -- the inverse of
// yuv.hip.  Not part of the reference, which writes no YUV.
//
// Arithmetic (integer after the quantizer, so the output is bit-exact against
// the numpy statement in tests/yuv_cases.py): every channel is clamped to
// [0, 1] (NaN -> 0), scaled by 255, 0.5 added and truncated -- the inverse of
// i420_to_rgb's /255 for all 256 levels; luma is BT.601 limited range at 20
// bits per pixel; chroma is taken from the SUM of the four quantized pixels of
// a 2x2 block at 22 bits, one rounding.  The largest accumulator is
// 1 008 498 544 < 2^31 and none is negative: int32 and a plain shift.
//
// Two layouts, same bytes.  Vector (W % 8 == 0, rgb 16-byte and out / ref
// 8-byte aligned: then every plane and frame starts aligned): one lane per
// 2 rows x 8 columns, 12 dwordx4 loads issued before first use, two 8-byte Y
// stores, one 4-byte U and one 4-byte V store.  Bytewise (everything else:
// for H*W/4 odd the V plane and every second frame start at odd or 2-mod-4
// offsets): one lane per 2x2 block, dword loads and byte stores.  HBM-bound:
// 12 B read + 1.5 B written per pixel (+1.5 B read with ref).
//
// With ref, squared byte differences are summed in integers per lane, then by
// wave, then by block; a block lies inside one frame and issues one 64-bit
// atomic add per plane, so the sums are exact and run-to-run identical.
#include "common.h"

namespace gsvc {

namespace {

constexpr int kYR = 269484, kYG = 528482, kYB = 102760;
constexpr int kUR = -155188, kUG = -305135, kUB = 460324;
constexpr int kVR = 460324, kVG = -385875, kVB = -74448;
constexpr int kYShift = 20, kCShift = 22;
constexpr int kMaxGridX = 4096;   // blocks per frame; the rest by grid stride
constexpr int kMaxGridY = 65535;  // frames per launch

__device__ __forceinline__ int quant8(float x) {
    const float c = fminf(fmaxf(x, 0.0f), 1.0f);
    return (int)__fadd_rn(__fmul_rn(c, 255.0f), 0.5f);
}

__device__ __forceinline__ int sat8(int x) { return x < 0 ? 0 : (x > 255 ? 255 : x); }

__device__ __forceinline__ int luma(int r, int g, int b) {
    return sat8((kYR * r + kYG * g + kYB * b + (16 << kYShift) + (1 << (kYShift - 1))) >> kYShift);
}

__device__ __forceinline__ int chroma(int cr, int cg, int cb, int rs, int gs, int bs) {
    return sat8((cr * rs + cg * gs + cb * bs + (128 << kCShift) + (1 << (kCShift - 1))) >> kCShift);
}

__device__ __forceinline__ unsigned sqdiff(int a, int b) {
    const int d = a - b;
    return (unsigned)(d * d);
}

// Four values in [0, 255] as one little-endian word.  The empty asm keeps the
// clamped values opaque: left to itself hipcc folds shift, clamp and the first
// two bytes' packing into gfx950's v_ashr_pk_u8_i32 and ORs bytes 2 and 3 into
// its result as if the upper half of that result were zero; on the MI355X the
// words then came back with bytes 2 and 3 wrong (tests/test_yuv_out_gpu.py).
__device__ __forceinline__ unsigned pack4(int a, int b, int c, int d) {
    asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
    return (unsigned)a | (unsigned)b << 8 | (unsigned)c << 16 | (unsigned)d << 24;
}

__device__ __forceinline__ int byte_of(unsigned word, int k) { return (int)((word >> (8 * k)) & 255u); }

// kVec: one lane per 2 rows x 8 columns, else per 2x2 block.  grid (blocks of
// one frame, frames); frame0: the first frame of this launch.
template <bool kVec, bool kRef>
__global__ __launch_bounds__(256) void rgb_to_i420_kernel(const float *__restrict__ rgb, int h, int w,
                                                          unsigned char *__restrict__ out,
                                                          const unsigned char *__restrict__ ref,
                                                          unsigned long long *__restrict__ sse,
                                                          int frame0) {
    constexpr int kCols = kVec ? 8 : 2;
    const size_t f = (size_t)frame0 + blockIdx.y;
    const size_t plane = (size_t)h * w, cplane = plane / 4, fsize = plane + 2 * cplane;
    const float *src = rgb + f * 3 * plane;
    unsigned char *dst = out + f * fsize;
    const unsigned char *rf = kRef ? ref + f * fsize : nullptr;
    const int hw = w / 2, upr = w / kCols;  // units per row pair
    const long long units = (long long)(h / 2) * upr;
    unsigned long long acc[3] = {0ull, 0ull, 0ull};

    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < units;
         t += (long long)gridDim.x * 256) {
        const int i2 = (int)(t / upr), k = (int)(t - (long long)i2 * upr);
        const size_t p0 = (size_t)(2 * i2) * w + (size_t)k * kCols;   // top row's first pixel
        const size_t c0 = plane + (size_t)i2 * hw + (size_t)k * (kCols / 2);  // its U byte
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
                uint2 wy[2];
                unsigned wc[2];
#pragma unroll
                for (int r = 0; r < 2; ++r)
                    wy[r] = *reinterpret_cast<const uint2 *>(rf + p0 + (size_t)r * w);
                wc[0] = *reinterpret_cast<const unsigned *>(rf + c0);
                wc[1] = *reinterpret_cast<const unsigned *>(rf + c0 + cplane);
#pragma unroll
                for (int r = 0; r < 2; ++r) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        ry[r][j] = byte_of(wy[r].x, j);
                        ry[r][4 + j] = byte_of(wy[r].y, j);
                        rc[r][j] = byte_of(wc[r], j);
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const float4 a = v[c][r][0], b = v[c][r][1];
                    q[c][r][0] = quant8(a.x);
                    q[c][r][1] = quant8(a.y);
                    q[c][r][2] = quant8(a.z);
                    q[c][r][3] = quant8(a.w);
                    q[c][r][4] = quant8(b.x);
                    q[c][r][5] = quant8(b.y);
                    q[c][r][6] = quant8(b.z);
                    q[c][r][7] = quant8(b.w);
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
                    for (int j = 0; j < 2; ++j) ry[r][j] = rf[p0 + (size_t)r * w + j];
                rc[0][0] = rf[c0];
                rc[1][0] = rf[c0 + cplane];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int j = 0; j < 2; ++j) q[c][r][j] = quant8(v[c][r][j]);
        }

        int y[2][kCols], uv[2][kCols / 2];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < kCols; ++j) y[r][j] = luma(q[0][r][j], q[1][r][j], q[2][r][j]);
#pragma unroll
        for (int j = 0; j < kCols / 2; ++j) {
            int s[3];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                s[c] = (q[c][0][2 * j] + q[c][0][2 * j + 1]) + (q[c][1][2 * j] + q[c][1][2 * j + 1]);
            uv[0][j] = chroma(kUR, kUG, kUB, s[0], s[1], s[2]);
            uv[1][j] = chroma(kVR, kVG, kVB, s[0], s[1], s[2]);
        }

        if constexpr (kVec) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                uint2 o;
                o.x = pack4(y[r][0], y[r][1], y[r][2], y[r][3]);
                o.y = pack4(y[r][4], y[r][5], y[r][6], y[r][7]);
                *reinterpret_cast<uint2 *>(dst + p0 + (size_t)r * w) = o;
            }
#pragma unroll
            for (int p = 0; p < 2; ++p)
                *reinterpret_cast<unsigned *>(dst + c0 + p * cplane) =
                    pack4(uv[p][0], uv[p][1], uv[p][2], uv[p][3]);
        } else {
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int j = 0; j < 2; ++j) dst[p0 + (size_t)r * w + j] = (unsigned char)y[r][j];
            dst[c0] = (unsigned char)uv[0][0];
            dst[c0 + cplane] = (unsigned char)uv[1][0];
        }

        if constexpr (kRef) {
            unsigned d[3] = {0u, 0u, 0u};  // <= 16 * 255^2 per unit
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int j = 0; j < kCols; ++j) d[0] += sqdiff(y[r][j], ry[r][j]);
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int j = 0; j < kCols / 2; ++j) d[1 + p] += sqdiff(uv[p][j], rc[p][j]);
#pragma unroll
            for (int p = 0; p < 3; ++p) acc[p] += d[p];
        }
    }

    if constexpr (kRef) {  // every lane arrives: the loop has no early exit
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

template <bool kVec, bool kRef>
void launch(int frames, const float *rgb, int h, int w, unsigned char *out, const unsigned char *ref,
            unsigned long long *sse, hipStream_t s) {
    const long long units = (long long)(h / 2) * (w / (kVec ? 8 : 2));
    const long long blocks = (units + 255) / 256;
    const unsigned gx = (unsigned)(blocks < kMaxGridX ? blocks : kMaxGridX);
    for (int f0 = 0; f0 < frames; f0 += kMaxGridY) {
        const int fy = frames - f0 < kMaxGridY ? frames - f0 : kMaxGridY;
        hipLaunchKernelGGL((rgb_to_i420_kernel<kVec, kRef>), dim3(gx, (unsigned)fy), dim3(256), 0, s, rgb,
                           h, w, out, ref, sse, f0);
    }
}

}  // namespace

}  // namespace gsvc

using namespace gsvc;

extern "C" int gsvc_rgb_to_i420(int frames, const float *rgb, int height, int width, unsigned char *out,
                                const unsigned char *ref, unsigned long long *sse, void *stream) {
    if (frames <= 0) return set_error(GSVC_ERR_ARG, "rgb_to_i420: frames = %d, must be positive", frames);
    if (height <= 0 || width <= 0 || (height & 1) || (width & 1))
        return set_error(GSVC_ERR_ARG, "rgb_to_i420: height and width must be positive and even");
    if (!rgb || !out) return set_error(GSVC_ERR_ARG, "rgb_to_i420: missing buffer");
    if (ref && !sse) return set_error(GSVC_ERR_ARG, "rgb_to_i420: ref needs sse");
    hipStream_t s = (hipStream_t)stream;
    if (ref) {
        const int rc = dev_zero(sse, (size_t)frames * 3 * sizeof(unsigned long long), s);
        if (rc) return rc;
    }
    const uintptr_t bytes_at = (uintptr_t)out | (uintptr_t)ref;
    const bool vec = (width % 8 == 0) && ((uintptr_t)rgb & 15u) == 0 && (bytes_at & 7u) == 0;
    if (vec) {
        if (ref) launch<true, true>(frames, rgb, height, width, out, ref, sse, s);
        else launch<true, false>(frames, rgb, height, width, out, nullptr, nullptr, s);
    } else {
        if (ref) launch<false, true>(frames, rgb, height, width, out, ref, sse, s);
        else launch<false, false>(frames, rgb, height, width, out, nullptr, nullptr, s);
    }
    return check_launch("rgb_to_i420");
}
