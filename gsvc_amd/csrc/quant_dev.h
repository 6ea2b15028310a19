// Device functions of the compression stage shared by quant.hip (the
// quantizer's forward / backward, the stream codec) and quant_train.hip (the
// fused quantized training step): one op sequence, so both give identical bits
// (DESIGN.md §13 "Operation orders", §13c).
#pragma once

#include <algorithm>

#include "stream.h"

namespace gsvc {

constexpr int kQuantBlock = 256;
constexpr int kQuantMaxBlocks = 1024;
constexpr int kQuantSums = 8;  // floats per block partial (6 used by the backward, 2 by the forward)
constexpr int kQMax = 63;      // 6-bit codes
constexpr int kCodewords = 8, kStages = 2;

inline int quant_blocks(int n) { return n < 1 ? 1 : std::min(ceil_div(n, kQuantBlock), kQuantMaxBlocks); }

// The decoder's arithmetic: half bits / codes / codewords -> xq, Lq, cq and the
// pre-bound Cholesky entries (what a following delta frame adds).
struct Recon {
    float xq[2], Lq[3], Lpre[3], cq[3];
};

__device__ __forceinline__ Recon reconstruct(_Float16 h0, _Float16 h1, const int code[3],
                                             const float scale[3], const float beta[3],
                                             const float bound[3], const float e0[3],
                                             const float e1[3], bool delta, const float px[2],
                                             const float pL[3], const float pc[3]) {
    Recon r;
    r.xq[0] = (float)h0;
    r.xq[1] = (float)h1;
    if (delta) {
        r.xq[0] = r.xq[0] + px[0];
        r.xq[1] = r.xq[1] + px[1];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float deq = __fadd_rn(__fmul_rn((float)code[k], scale[k]), beta[k]);
        const float lb = deq + bound[k];
        r.Lq[k] = delta ? lb + pL[k] : lb;
        r.Lpre[k] = delta ? deq + pL[k] : deq;
        const float c = e0[k] + e1[k];
        r.cq[k] = delta ? c + pc[k] : c;
    }
    return r;
}

__device__ __forceinline__ float quant_raw(float c, float scale, float beta) {
    return __fdiv_rn(c - beta, scale);
}
__device__ __forceinline__ float quant_code(float raw) {
    return rintf(fminf(fmaxf(raw, 0.0f), (float)kQMax));
}

// nearest codeword of one stage: index (lowest of equal distances), distance
__device__ __forceinline__ int vq_nearest(const float r[3], const float *__restrict__ cb,
                                          float &dmin) {
    int best = 0;
    float bd = 0.0f;
#pragma unroll
    for (int j = 0; j < kCodewords; ++j) {
        const float a = r[0] - cb[3 * j], b = r[1] - cb[3 * j + 1], c = r[2] - cb[3 * j + 2];
        const float d = (a * a + b * b) + c * c;
        if (j == 0 || d < bd) {
            bd = d;
            best = j;
        }
    }
    dmin = bd;
    return best;
}

// One splat of the straight-through backward (gsvc_quant_params_backward):
// vch = v_cholesky, g = v_features, and the splat's terms added to
// sums = {v_scale[3], v_beta[3]}.  cv: the Cholesky entries, vL / vq: the
// gradients of Lq / cq; with ``commit``, fv are the features, i0 / i1 their
// codes and vc0 / vc1 the gradients of the two commitment sums.
__device__ __forceinline__ void quant_backward_splat(const float cv[3], const float vL[3],
                                                     const float vq[3], const float scale[3],
                                                     const float beta[3], bool commit,
                                                     const float fv[3],
                                                     const float *__restrict__ cb, int i0, int i1,
                                                     float vc0, float vc1, float vch[3],
                                                     float g[3], float (&sums)[6]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float raw = quant_raw(cv[k], scale[k], beta[k]);
        const float q = quant_code(raw);
        const float mask = (raw >= 0.0f && raw <= (float)kQMax) ? 1.0f : 0.0f;
        vch[k] = vL[k] * mask;
        sums[k] = sums[k] + vL[k] * (q - mask * raw);
        sums[3 + k] = sums[3 + k] + vL[k] * (1.0f - mask);
    }
    // each stage is straight-through on its own residual: d cq / d f = 2
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = 2.0f * vq[k];
    if (commit) {
        const float *cb1 = cb + 3 * kCodewords;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float r1 = fv[k] - cb[3 * i0 + k];  // stage 0: r0 - e0, also stage 1's residual
            const float t0 = vc0 * (2.0f * r1);
            const float t1 = vc1 * (2.0f * (r1 - cb1[3 * i1 + k]));
            g[k] = g[k] + (t0 + t1);
        }
    }
}

// Block partial of K per-lane sums -> partials[block * kQuantSums + k].
template <int K>
__device__ __forceinline__ void block_partial(float (&v)[K], float *__restrict__ partials) {
    __shared__ float wave_sums[kQuantBlock / 64][K];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v[k] = v[k] + __shfl_xor(v[k], m, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) wave_sums[wave][k] = v[k];
    __syncthreads();
    if (threadIdx.x < K) {
        float s = wave_sums[0][threadIdx.x];
        for (int w = 1; w < kQuantBlock / 64; ++w) s = s + wave_sums[w][threadIdx.x];
        partials[blockIdx.x * kQuantSums + threadIdx.x] = s;
    }
}

// Column p[0], p[stride], ... of nblocks block partials summed in block order.
// The loads go 16 ahead of the adds: the chain is then the additions, not
// every load's latency (the order of the additions, and so the bits, are those
// of the plain loop).
template <typename V>
__device__ __forceinline__ V sum_block_order(const V *__restrict__ p, int nblocks, int stride) {
    V s = p[0];
    for (int b = 1; b < nblocks; b += 16) {
        V v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = b + k < nblocks ? p[(size_t)(b + k) * stride] : V(0);
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (b + k < nblocks) s = s + v[k];
    }
    return s;
}

// quant.hip: the training variant of the quantizer forward (quant_forward_kernel
// with its commitment sums) and the combine of its partials into commit_sums
// [2], for gsvc_quant_params_forward and the fused step.  The caller has
// validated the arguments (num_points >= 1; partials of quant_blocks(n) *
// kQuantSums floats); returns a gsvc status.
int launch_quant_forward_train(const char *what, int num_points, const float *xyz,
                               const float *cholesky, const float *features, const float *scale,
                               const float *beta, const float *codebooks,
                               const float *cholesky_bound, const float *p_xyz,
                               const float *p_cholesky, const float *p_features, float *xq,
                               float *Lq, float *cq, unsigned char *codes_chol,
                               unsigned char *codes_rgb, float *partials, float *commit_sums,
                               hipStream_t s);

}  // namespace gsvc
