// Compression stage (gfx950): quantized frame parameters and the packed stream.
//
// Reference: GaussianSplats_Compress.py:71-84,165-179 (forward_quantize) over
// quantize.py:15-87 -- positions through fp16, Cholesky entries through a
// learned 6-bit uniform quantizer, colours through a 2-stage residual vector
// quantizer of 8 codewords per stage; a non-key frame adds the previous
// frame's parameters.  Streaming per-splat kernels, one splat per lane.
//
// Op sequence (-ffp-contract=off, every op its own rounding):
//   xq  = float(half_rne(x))                                   (+ p_xyz)
//   raw = (c - beta) / scale                 IEEE division
//   q   = rint(min(max(raw, 0), 63))         round half to even; a NaN gives 0
//   Lq  = ((q * scale + beta) + bound)                         (+ p_cholesky)
//   d_j = ((r0-e_j0)^2 + (r1-e_j1)^2) + (r2-e_j2)^2   lowest j of the smallest
//   stage 0 on r = f, stage 1 on r = f - e0;  cq = (e0 + e1)   (+ p_features)
// The unpack kernel rebuilds xq, Lq, cq from the stored half / codes with the
// same device function (reconstruct), so the decoder's bits are the encoder's.
//
// Reductions (the commitment sums, v_scale, v_beta) have a fixed order and no
// float atomics: a lane adds its splats in index order (a grid of at most
// kQuantMaxBlocks blocks strides over N), a wave folds by xor-shuffles 32..1,
// lane 0..K-1 of the block adds the 4 wave sums in order and stores the block
// partial, and a second one-block launch adds the partials in block order.
#include "quant_dev.h"

namespace gsvc {

// stream layout: stream.h; the shared device functions: quant_dev.h
static_assert(kOffCodebooks + 4 * 3 * kStages * kCodewords <= kHeaderBytes, "header layout");

// out_a[0..na) and out_b[0..nb) = the partials' columns summed in block order
__global__ __launch_bounds__(64) void quant_combine_kernel(const float *__restrict__ partials,
                                                           int nblocks, float *out_a, int na,
                                                           float *out_b, int nb) {
    const int k = threadIdx.x;
    if (k >= na + nb) return;
    const float s = sum_block_order(partials + k, nblocks, kQuantSums);
    if (k < na)
        out_a[k] = s;
    else
        out_b[k - na] = s;
}

template <bool kTrain>
__global__ __launch_bounds__(kQuantBlock) void quant_forward_kernel(
    int n, const float *__restrict__ xyz, const float *__restrict__ chol,
    const float *__restrict__ feat, const float *__restrict__ scale_p,
    const float *__restrict__ beta_p, const float *__restrict__ cb,
    const float *__restrict__ bound_p, const float *__restrict__ p_xyz,
    const float *__restrict__ p_chol, const float *__restrict__ p_feat, float *__restrict__ xq,
    float *__restrict__ Lq, float *__restrict__ cq, unsigned char *__restrict__ codes_chol,
    unsigned char *__restrict__ codes_rgb, float *__restrict__ partials) {
    const float scale[3] = {scale_p[0], scale_p[1], scale_p[2]};
    const float beta[3] = {beta_p[0], beta_p[1], beta_p[2]};
    const float bound[3] = {bound_p[0], bound_p[1], bound_p[2]};
    const bool delta = p_xyz != nullptr;
    float sums[2] = {0.0f, 0.0f};
    for (long long i = (long long)blockIdx.x * kQuantBlock + threadIdx.x; i < n;
         i += (long long)gridDim.x * kQuantBlock) {
        float x[2], cv[3], r0[3];
        ld_row<2>(xyz, i, x);
        ld_row<3>(chol, i, cv);
        ld_row<3>(feat, i, r0);
        const _Float16 h0 = (_Float16)x[0], h1 = (_Float16)x[1];
        int code[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) code[k] = (int)quant_code(quant_raw(cv[k], scale[k], beta[k]));
        float d0, d1;
        const int i0 = vq_nearest(r0, cb, d0);
        const float e0[3] = {cb[3 * i0], cb[3 * i0 + 1], cb[3 * i0 + 2]};
        const float r1[3] = {r0[0] - e0[0], r0[1] - e0[1], r0[2] - e0[2]};
        const float *cb1 = cb + 3 * kCodewords;
        const int i1 = vq_nearest(r1, cb1, d1);
        const float e1[3] = {cb1[3 * i1], cb1[3 * i1 + 1], cb1[3 * i1 + 2]};
        float px[2] = {0.0f, 0.0f}, pL[3] = {0.0f, 0.0f, 0.0f}, pc[3] = {0.0f, 0.0f, 0.0f};
        if (delta) {
            ld_row<2>(p_xyz, i, px);
            ld_row<3>(p_chol, i, pL);
            ld_row<3>(p_feat, i, pc);
        }
        const Recon r = reconstruct(h0, h1, code, scale, beta, bound, e0, e1, delta, px, pL, pc);
        st_row<2>(xq, i, r.xq);
        st_row<3>(Lq, i, r.Lq);
        st_row<3>(cq, i, r.cq);
        codes_chol[3 * i] = (unsigned char)code[0];
        codes_chol[3 * i + 1] = (unsigned char)code[1];
        codes_chol[3 * i + 2] = (unsigned char)code[2];
        codes_rgb[2 * i] = (unsigned char)i0;
        codes_rgb[2 * i + 1] = (unsigned char)i1;
        if (kTrain) {
            sums[0] = sums[0] + d0;
            sums[1] = sums[1] + d1;
        }
    }
    if (kTrain) block_partial(sums, partials);
}

__global__ __launch_bounds__(kQuantBlock) void quant_backward_kernel(
    int n, const float *__restrict__ chol, const float *__restrict__ feat,
    const float *__restrict__ scale_p, const float *__restrict__ beta_p,
    const float *__restrict__ cb, const unsigned char *__restrict__ codes_rgb,
    const float *__restrict__ v_xq, const float *__restrict__ v_Lq,
    const float *__restrict__ v_cq, const float *__restrict__ v_commit,
    float *__restrict__ v_xyz, float *__restrict__ v_chol, float *__restrict__ v_feat,
    float *__restrict__ partials) {
    const float scale[3] = {scale_p[0], scale_p[1], scale_p[2]};
    const float beta[3] = {beta_p[0], beta_p[1], beta_p[2]};
    const bool commit = v_commit != nullptr;
    const float vc0 = commit ? v_commit[0] : 0.0f, vc1 = commit ? v_commit[1] : 0.0f;
    float sums[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // v_scale[3], v_beta[3]
    for (long long i = (long long)blockIdx.x * kQuantBlock + threadIdx.x; i < n;
         i += (long long)gridDim.x * kQuantBlock) {
        float vx[2], cv[3], vL[3], vc[3];
        ld_row<2>(v_xq, i, vx);
        st_row<2>(v_xyz, i, vx);
        ld_row<3>(chol, i, cv);
        ld_row<3>(v_Lq, i, vL);
        ld_row<3>(v_cq, i, vc);
        float fv[3] = {0.0f, 0.0f, 0.0f};
        int i0 = 0, i1 = 0;
        if (commit) {
            ld_row<3>(feat, i, fv);
            i0 = codes_rgb[2 * i] & (kCodewords - 1), i1 = codes_rgb[2 * i + 1] & (kCodewords - 1);
        }
        float vch[3], g[3];
        quant_backward_splat(cv, vL, vc, scale, beta, commit, fv, cb, i0, i1, vc0, vc1, vch, g, sums);
        st_row<3>(v_chol, i, vch);
        st_row<3>(v_feat, i, g);
    }
    block_partial(sums, partials);
}

// planes: A = n x {half x, half y} (4 n bytes), then B = n x 3 bytes
// c0 | c1 << 6 | c2 << 12 | i0 << 18 | i1 << 21, little-endian.
__global__ __launch_bounds__(kQuantBlock) void pack_kernel(
    int n, const float *__restrict__ xyz, const unsigned char *__restrict__ codes_chol,
    const unsigned char *__restrict__ codes_rgb, unsigned char *__restrict__ planes) {
    const long long i = (long long)blockIdx.x * kQuantBlock + threadIdx.x;
    if (i >= n) return;
    float x[2];
    ld_row<2>(xyz, i, x);
    const _Float16 h0 = (_Float16)x[0], h1 = (_Float16)x[1];
    unsigned short b0, b1;
    __builtin_memcpy(&b0, &h0, 2);
    __builtin_memcpy(&b1, &h1, 2);
    unsigned char *a = planes + 4 * i;
    a[0] = (unsigned char)(b0 & 0xff);
    a[1] = (unsigned char)(b0 >> 8);
    a[2] = (unsigned char)(b1 & 0xff);
    a[3] = (unsigned char)(b1 >> 8);
    const unsigned w = (codes_chol[3 * i] & 63u) | (codes_chol[3 * i + 1] & 63u) << 6 |
                       (codes_chol[3 * i + 2] & 63u) << 12 | (codes_rgb[2 * i] & 7u) << 18 |
                       (codes_rgb[2 * i + 1] & 7u) << 21;
    unsigned char *b = planes + 4ll * n + 3 * i;
    b[0] = (unsigned char)(w & 0xff);
    b[1] = (unsigned char)((w >> 8) & 0xff);
    b[2] = (unsigned char)((w >> 16) & 0xff);
}

__device__ __forceinline__ float rd_f32(const unsigned char *p) {
    return __uint_as_float(rd_u32(p));
}

// One launch for a concatenation of F frames: lane i walks the frames in
// order and carries splat i's decoded pre-activation parameters from frame to
// frame (a delta frame of n splats adds its predecessor's first n; the host
// checked n <= the predecessor's count).  The walk re-checks every frame
// against total_bytes / total_splats, so a device copy that differs from the
// validated host copy cannot make it read or write out of bounds.
__global__ __launch_bounds__(kQuantBlock) void unpack_kernel(
    int nframes, const unsigned char *__restrict__ stream, long long total_bytes,
    long long total_splats, const float *__restrict__ bound_p, const float *__restrict__ prev_xyz,
    const float *__restrict__ prev_chol, const float *__restrict__ prev_feat, int prev_n,
    float *__restrict__ xq, float *__restrict__ Lq, float *__restrict__ cq,
    float *__restrict__ Lpre) {
    const long long i = (long long)blockIdx.x * kQuantBlock + threadIdx.x;
    const float bound[3] = {bound_p[0], bound_p[1], bound_p[2]};
    float px[2] = {0.0f, 0.0f}, pL[3] = {0.0f, 0.0f, 0.0f}, pc[3] = {0.0f, 0.0f, 0.0f};
    long long have = 0;  // splats of the previous frame this walk has decoded
    if (prev_n > 0) {
        have = prev_n;
        if (i < prev_n) {
            px[0] = prev_xyz[2 * i], px[1] = prev_xyz[2 * i + 1];
#pragma unroll
            for (int k = 0; k < 3; ++k) pL[k] = prev_chol[3 * i + k], pc[k] = prev_feat[3 * i + k];
        }
    }
    long long off = 0, so = 0;
    for (int f = 0; f < nframes; ++f) {
        if (off + kHeaderBytes > total_bytes) break;
        const unsigned char *hdr = stream + off;
        const long long n = (long long)(int)rd_u32(hdr + kOffN);
        const bool delta = (rd_u32(hdr + kOffFlags) & 1u) != 0;
        if (n < 0 || off + kHeaderBytes + kSplatBytes * n > total_bytes || so + n > total_splats ||
            (delta && n > have))
            break;
        if (i < n) {
            float scale[3], beta[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                scale[k] = rd_f32(hdr + kOffScale + 4 * k);
                beta[k] = rd_f32(hdr + kOffBeta + 4 * k);
            }
            const unsigned char *a = hdr + kHeaderBytes + 4 * i;
            const unsigned char *b = hdr + kHeaderBytes + 4 * n + 3 * i;
            const unsigned ha = rd_u32(a);
            const unsigned short b0 = (unsigned short)(ha & 0xffff), b1 = (unsigned short)(ha >> 16);
            _Float16 h0, h1;
            __builtin_memcpy(&h0, &b0, 2);
            __builtin_memcpy(&h1, &b1, 2);
            const unsigned w = (unsigned)b[0] | (unsigned)b[1] << 8 | (unsigned)b[2] << 16;
            const int code[3] = {(int)(w & 63u), (int)((w >> 6) & 63u), (int)((w >> 12) & 63u)};
            const int i0 = (int)((w >> 18) & 7u), i1 = (int)((w >> 21) & 7u);
            const unsigned char *cb0 = hdr + kOffCodebooks + 12 * i0;
            const unsigned char *cb1 = hdr + kOffCodebooks + 12 * (kCodewords + i1);
            const float e0[3] = {rd_f32(cb0), rd_f32(cb0 + 4), rd_f32(cb0 + 8)};
            const float e1[3] = {rd_f32(cb1), rd_f32(cb1 + 4), rd_f32(cb1 + 8)};
            const Recon r = reconstruct(h0, h1, code, scale, beta, bound, e0, e1, delta, px, pL, pc);
            const long long o = so + i;
            st_row<2>(xq, o, r.xq);
            st_row<3>(Lq, o, r.Lq);
            st_row<3>(cq, o, r.cq);
            if (Lpre) st_row<3>(Lpre, o, r.Lpre);
            px[0] = r.xq[0], px[1] = r.xq[1];
#pragma unroll
            for (int k = 0; k < 3; ++k) pL[k] = r.Lpre[k], pc[k] = r.cq[k];
        }
        have = n;
        off += kHeaderBytes + kSplatBytes * n;
        so += n;
    }
}

// the forward's training variant and its combine (quant_dev.h)
int launch_quant_forward_train(const char *what, int num_points, const float *xyz,
                               const float *cholesky, const float *features, const float *scale,
                               const float *beta, const float *codebooks,
                               const float *cholesky_bound, const float *p_xyz,
                               const float *p_cholesky, const float *p_features, float *xq,
                               float *Lq, float *cq, unsigned char *codes_chol,
                               unsigned char *codes_rgb, float *partials, float *commit_sums,
                               hipStream_t s) {
    const int blocks = quant_blocks(num_points);
    hipLaunchKernelGGL(quant_forward_kernel<true>, dim3(blocks), dim3(kQuantBlock), 0, s, num_points,
                       xyz, cholesky, features, scale, beta, codebooks, cholesky_bound, p_xyz,
                       p_cholesky, p_features, xq, Lq, cq, codes_chol, codes_rgb, partials);
    int rc = check_launch(what);
    if (rc) return rc;
    hipLaunchKernelGGL(quant_combine_kernel, dim3(1), dim3(64), 0, s, (const float *)partials,
                       blocks, commit_sums, 2, (float *)nullptr, 0);
    return check_launch(what);
}

// the walk's launch, for gsvc_unpack_splats and gsvc_unpack_stream (stream.h)
int launch_unpack_walk(const char *what, int num_frames, const unsigned char *stream_dev,
                       long long total_bytes, long long total_splats, long long nmax,
                       const float *cholesky_bound, const float *prev_xyz,
                       const float *prev_cholesky, const float *prev_features, int prev_points,
                       float *xq, float *Lq, float *cq, float *Lpre, hipStream_t s) {
    if (nmax > 0x7fffffffll - kQuantBlock) return set_error(GSVC_ERR_ARG, "%s: frame too large", what);
    hipLaunchKernelGGL(unpack_kernel, dim3(ceil_div((int)nmax, kQuantBlock)), dim3(kQuantBlock), 0, s,
                       num_frames, stream_dev, total_bytes, total_splats, cholesky_bound, prev_xyz,
                       prev_cholesky, prev_features, prev_points, xq, Lq, cq, Lpre);
    return check_launch(what);
}

}  // namespace gsvc

using namespace gsvc;

extern "C" size_t gsvc_quant_workspace_bytes(int num_points) {
    return (size_t)quant_blocks(num_points) * kQuantSums * sizeof(float);
}

extern "C" int gsvc_quant_params_forward(
    int num_points, const float *xyz, const float *cholesky, const float *features,
    const float *scale, const float *beta, const float *codebooks, const float *cholesky_bound,
    const float *p_xyz, const float *p_cholesky, const float *p_features, float *xq, float *Lq,
    float *cq, unsigned char *codes_chol, unsigned char *codes_rgb, float *commit_sums,
    void *workspace, size_t workspace_bytes, void *stream) {
    if (num_points < 0) return set_error(GSVC_ERR_ARG, "quant_params_forward: num_points < 0");
    if (!scale || !beta || !codebooks || !cholesky_bound)
        return set_error(GSVC_ERR_ARG, "quant_params_forward: null quantizer tables");
    const int np = (p_xyz != nullptr) + (p_cholesky != nullptr) + (p_features != nullptr);
    if (np != 0 && np != 3)
        return set_error(GSVC_ERR_ARG, "quant_params_forward: p_xyz, p_cholesky, p_features go together");
    if (num_points > 0 && (!xyz || !cholesky || !features || !xq || !Lq || !cq || !codes_chol || !codes_rgb))
        return set_error(GSVC_ERR_ARG, "quant_params_forward: null tensor");
    const int blocks = quant_blocks(num_points);
    if (commit_sums && (!workspace || workspace_bytes < gsvc_quant_workspace_bytes(num_points)))
        return set_error(GSVC_ERR_WORKSPACE, "quant_params_forward: workspace of %zu bytes, need %zu",
                         workspace_bytes, gsvc_quant_workspace_bytes(num_points));
    hipStream_t s = (hipStream_t)stream;
    if (num_points == 0) {
        if (commit_sums) return dev_zero(commit_sums, 2 * sizeof(float), s);
        return GSVC_OK;
    }
    if (commit_sums)
        return launch_quant_forward_train("quant_params_forward", num_points, xyz, cholesky, features,
                                          scale, beta, codebooks, cholesky_bound, p_xyz, p_cholesky,
                                          p_features, xq, Lq, cq, codes_chol, codes_rgb,
                                          (float *)workspace, commit_sums, s);
    hipLaunchKernelGGL(quant_forward_kernel<false>, dim3(blocks), dim3(kQuantBlock), 0, s, num_points,
                       xyz, cholesky, features, scale, beta, codebooks, cholesky_bound, p_xyz,
                       p_cholesky, p_features, xq, Lq, cq, codes_chol, codes_rgb, (float *)nullptr);
    return check_launch("quant_params_forward");
}

extern "C" int gsvc_quant_params_backward(
    int num_points, const float *cholesky, const float *features, const float *scale,
    const float *beta, const float *codebooks, const unsigned char *codes_rgb, const float *v_xq,
    const float *v_Lq, const float *v_cq, const float *v_commit, float *v_xyz, float *v_cholesky,
    float *v_features, float *v_scale, float *v_beta, void *workspace, size_t workspace_bytes,
    void *stream) {
    if (num_points < 0) return set_error(GSVC_ERR_ARG, "quant_params_backward: num_points < 0");
    if (!scale || !beta || !v_scale || !v_beta)
        return set_error(GSVC_ERR_ARG, "quant_params_backward: null scale / beta");
    if (v_commit && (!codebooks || (num_points > 0 && (!codes_rgb || !features))))
        return set_error(GSVC_ERR_ARG, "quant_params_backward: the commitment term needs features, "
                                       "codebooks and codes_rgb");
    if (num_points > 0 && (!cholesky || !v_xq || !v_Lq || !v_cq || !v_xyz || !v_cholesky || !v_features))
        return set_error(GSVC_ERR_ARG, "quant_params_backward: null tensor");
    if (!workspace || workspace_bytes < gsvc_quant_workspace_bytes(num_points))
        return set_error(GSVC_ERR_WORKSPACE, "quant_params_backward: workspace of %zu bytes, need %zu",
                         workspace_bytes, gsvc_quant_workspace_bytes(num_points));
    hipStream_t s = (hipStream_t)stream;
    if (num_points == 0) {
        int rc = dev_zero(v_scale, 3 * sizeof(float), s);
        return rc ? rc : dev_zero(v_beta, 3 * sizeof(float), s);
    }
    const int blocks = quant_blocks(num_points);
    float *partials = (float *)workspace;
    hipLaunchKernelGGL(quant_backward_kernel, dim3(blocks), dim3(kQuantBlock), 0, s, num_points,
                       cholesky, features, scale, beta, codebooks, codes_rgb, v_xq, v_Lq, v_cq,
                       v_commit, v_xyz, v_cholesky, v_features, partials);
    int rc = check_launch("quant_params_backward");
    if (rc) return rc;
    hipLaunchKernelGGL(quant_combine_kernel, dim3(1), dim3(64), 0, s, (const float *)partials, blocks,
                       v_scale, 3, v_beta, 3);
    return check_launch("quant_params_backward (combine)");
}

extern "C" int gsvc_pack_splats(int num_points, const float *xyz, const unsigned char *codes_chol,
                                const unsigned char *codes_rgb, unsigned char *planes, void *stream) {
    if (num_points < 0) return set_error(GSVC_ERR_ARG, "pack_splats: num_points < 0");
    if (num_points == 0) return GSVC_OK;
    if (!xyz || !codes_chol || !codes_rgb || !planes)
        return set_error(GSVC_ERR_ARG, "pack_splats: null tensor");
    hipLaunchKernelGGL(pack_kernel, dim3(ceil_div(num_points, kQuantBlock)), dim3(kQuantBlock), 0,
                       (hipStream_t)stream, num_points, xyz, codes_chol, codes_rgb, planes);
    return check_launch("pack_splats");
}

static unsigned host_u32(const unsigned char *p) { return rd_u32(p); }

extern "C" int gsvc_unpack_splats(int num_frames, const unsigned char *stream_host,
                                  const long long *frame_offsets, const unsigned char *stream_dev,
                                  const float *cholesky_bound, const float *prev_xyz,
                                  const float *prev_cholesky, const float *prev_features,
                                  int prev_points, float *xq, float *Lq, float *cq, float *Lpre,
                                  long long out_capacity, void *stream) {
    if (num_frames < 0) return set_error(GSVC_ERR_ARG, "unpack_splats: num_frames < 0");
    if (num_frames == 0) return GSVC_OK;
    if (!stream_host || !frame_offsets)
        return set_error(GSVC_ERR_ARG, "unpack_splats: null stream / frame_offsets");
    if (prev_points < 0 || (prev_points > 0 && (!prev_xyz || !prev_cholesky || !prev_features)))
        return set_error(GSVC_ERR_ARG, "unpack_splats: bad previous-frame arguments");
    if (frame_offsets[0] != 0) return set_error(GSVC_ERR_ARG, "unpack_splats: frame_offsets[0] != 0");
    long long total = 0, have = prev_points, nmax = 0;
    unsigned H = 0, W = 0;
    for (int f = 0; f < num_frames; ++f) {
        const long long off = frame_offsets[f], len = frame_offsets[f + 1] - off;
        if (len < kHeaderBytes)
            return set_error(GSVC_ERR_ARG, "unpack_splats: frame %d truncated (%lld bytes, header is %d)",
                             f, len, kHeaderBytes);
        const unsigned char *hdr = stream_host + off;
        if (host_u32(hdr + kOffMagic) != kStreamMagic)
            return set_error(GSVC_ERR_ARG, "unpack_splats: frame %d has a wrong magic 0x%08x", f,
                             host_u32(hdr + kOffMagic));
        if (host_u32(hdr + kOffVersion) != GSVC_STREAM_VERSION)
            return set_error(GSVC_ERR_ARG, "unpack_splats: frame %d has stream version %u, not %d", f,
                             host_u32(hdr + kOffVersion), GSVC_STREAM_VERSION);
        const long long n = (long long)(int)host_u32(hdr + kOffN);
        if (n < 0) return set_error(GSVC_ERR_ARG, "unpack_splats: frame %d has N < 0", f);
        if (len != kHeaderBytes + kSplatBytes * n)
            return set_error(GSVC_ERR_ARG, "unpack_splats: frame %d truncated or padded (%lld bytes, "
                                           "N = %lld needs %lld)", f, len, n, kHeaderBytes + kSplatBytes * n);
        const unsigned h = host_u32(hdr + kOffH), w = host_u32(hdr + kOffW);
        if (f == 0) H = h, W = w;
        if (h != H || w != W)
            return set_error(GSVC_ERR_ARG, "unpack_splats: frame %d is %ux%u, frame 0 %ux%u", f, h, w, H, W);
        const unsigned flags = host_u32(hdr + kOffFlags);
        if (flags & ~1u) return set_error(GSVC_ERR_ARG, "unpack_splats: frame %d has unknown flags", f);
        if (flags & 1u) {
            if (f == 0 && prev_points == 0)
                return set_error(GSVC_ERR_ARG, "unpack_splats: delta frame %d has no predecessor", f);
            if (n > have)
                return set_error(GSVC_ERR_ARG, "unpack_splats: delta frame %d has %lld splats, its "
                                               "predecessor %lld", f, n, have);
        }
        have = n;
        total += n;
        nmax = std::max(nmax, n);
    }
    if (total > out_capacity)
        return set_error(GSVC_ERR_ARG, "unpack_splats: %lld splats, outputs hold %lld", total, out_capacity);
    if (total == 0) return GSVC_OK;
    if (!stream_dev || !cholesky_bound || !xq || !Lq || !cq)
        return set_error(GSVC_ERR_ARG, "unpack_splats: null tensor");
    return launch_unpack_walk("unpack_splats", num_frames, stream_dev, frame_offsets[num_frames], total,
                              nmax, cholesky_bound, prev_xyz, prev_cholesky, prev_features, prev_points,
                              xq, Lq, cq, Lpre, (hipStream_t)stream);
}
