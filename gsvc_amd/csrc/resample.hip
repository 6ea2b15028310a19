// Batched frame render at any output size and window (gfx950): the frame
// models of gsvc_render_frames_sum evaluated at other sample positions.
//
// A frame model is the function the sum rasterizer computes: per 16x16 SOURCE
// tile, the tile's first <= 256 entries in splat-id order (forward.cu:569-571,
// 613), each contributing colour * min(1, opacity * exp(-sigma)) where
// sigma >= 0 and alpha >= 1/255.  The native render evaluates it at the
// integer coordinates (j, i) of the source grid; this one evaluates the SAME
// per-tile lists at the positions of a view (include/gsvc_amd.h: the sampling
// rule and its four tables), so an identity view gives the native bits, an
// integer crop the native render's window, and an odd integer upscale hits the
// native samples exactly.  Scaling the splats and rendering at the new size
// would re-bin them by the output grid's tiles and move the 256-entry cut, the
// radius rounding and the alpha cut.
//
// Two kernels: the frame projection of frame.hip at the SOURCE size (record
// slabs, counts parity, M and meta as gsvc_render_frames_sum), then
//   raster_resampled_kernel  one wave per (frame, source tile): the tile's
//                            ids sorted by tile_ids.h (slab, overflow ids or
//                            the bbox rebuild, as the native composite), their
//                            records gathered into LDS once, then the output
//                            samples the tile owns -- rows [row_start[ty],
//                            row_start[ty + 1]) x columns [col_start[tx],
//                            col_start[tx + 1]) -- walked 64 at a time as one
//                            flat index (lane = sample), every lane reading
//                            the staged records at a wave-uniform address.
// Lane use: a rectangle of R x C samples keeps R C / (64 ceil(R C / 64)) of
// the lanes busy whatever its shape (8 x 8 at half size, 32 x 32 at double
// size and 16 x 16 at the identity: all of them); consecutive lanes are
// consecutive columns of a row, so the plane stores coalesce along rows.
#include "frame.h"
#include "tile_ids.h"

namespace gsvc {

struct ResampleArgs {
    int tbx, ntiles, frames;
    int out_w, out_h;
    const float *sample_x, *sample_y;  // [out_w], [out_h]: model coordinates
    const int *col_start, *row_start;  // [tbx + 1], [tby + 1]
    int tby;
    const int *m_dev;
    int *meta_out;
    const float *bg;
    const float4 *slab;
    const int *slab_ovf;
    const unsigned *slab_counts;
    unsigned *slab_counts_clear;
    const float2 *cull_xys;
    const int *cull_radii;
    const float4 *rec;
    const int *frame_off;
    int counts_stride, m_stride;
    size_t slab_stride;
    float *out;
};

__device__ __forceinline__ float clamp01_keep_nan(float x) {
    // torch.clamp(x, 0, 1): NaN stays NaN
    return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
}

// (10 KB of LDS per wave: 16 waves per CU, 4 per SIMD)
__global__ __launch_bounds__(64) void raster_resampled_kernel(ResampleArgs A) {
    __shared__ float4 s_geo[kTilePix];  // x, y, a/2, b (the sort's bitmap before staging)
    __shared__ float4 s_col[kTilePix];  // c/2, opacity, r, g
    __shared__ float s_blu[kTilePix];   // b
    __shared__ int s_ids[kTilePix];     // the tile's sorted ids
    static_assert(sizeof(float4) * kTilePix >= sizeof(unsigned) * kSortWords, "bitmap in s_geo");
    const int lane = threadIdx.x & 63;
    int tile = xcd_runs<16>(blockIdx.x, A.ntiles * A.frames);
    const int b = tile / A.ntiles;
    tile -= b * A.ntiles;
    const float4 *slab = A.slab + b * A.slab_stride;
    const int *ovf = A.slab_ovf + (size_t)b * kOvfSlots * (size_t)A.ntiles;
    const unsigned *counts = A.slab_counts + (size_t)b * A.counts_stride;
    unsigned *counts_clear = A.slab_counts_clear + (size_t)b * A.counts_stride;
    const int m_val = A.m_dev[(size_t)b * A.m_stride];
    int n_all = (int)__builtin_amdgcn_readfirstlane(counts[tile]);
    if (lane == 0) {
        counts_clear[tile] = 0u;  // the next call's counts
        if (tile == 0) {
            A.meta_out[(size_t)b * A.m_stride] = m_val;
            A.meta_out[(size_t)b * A.m_stride + 1] = 0;
        }
    }
    const int ty = tile / A.tbx, tx = tile - ty * A.tbx;
    const int r0 = A.row_start[ty], r1 = A.row_start[ty + 1];
    const int c0 = A.col_start[tx], c1 = A.col_start[tx + 1];
    const int C = c1 - c0, total = (r1 - r0) * C;
    if (total <= 0) return;  // the tile owns no output sample (wave-uniform)
    // rasterize_sum.py:121-127: a frame without intersections is the background
    float3 init = make_float3(0.f, 0.f, 0.f);
    int n = 0;
    if (m_val < 1) {
        init = make_float3(A.bg[0], A.bg[1], A.bg[2]);
    } else {
        // the native composite's list: the slab's ids (slots past 256 from the
        // overflow ids) sorted, or past kCarryCap the first 256 by the bbox
        // rebuild over the frame's splats
        SegIds seg;
        seg.ids = nullptr;
        seg.recs = slab_rec(slab, A.ntiles, tile, kHeadSlots) - 3 * kHeadSlots;
        seg.head = slab_rec(slab, A.ntiles, tile, 0);
        seg.ovf = ovf + (size_t)tile * kOvfSlots;
        n = n_all > seg.cap()
                ? wave_brute_ids(A.cull_xys, A.cull_radii, A.frame_off[b], A.frame_off[b + 1], A.tbx,
                                 A.tby, tile, s_ids)
                : wave_sorted_tile_ids(seg, n_all, s_ids, reinterpret_cast<unsigned *>(s_geo));
        n = __builtin_amdgcn_readfirstlane(n);  // wave-uniform: a scalar entry loop
        for (int j = lane; j < n; j += 64) {
            const float4 *r = A.rec + 3 * (size_t)s_ids[j];
            const float4 g = r[0], c = r[1];
            const float bl = r[2].x;
            s_geo[j] = g;
            s_col[j] = c;
            s_blu[j] = bl;
        }
        wave_lds_sync();
    }
    const size_t plane = (size_t)A.out_w * (size_t)A.out_h;
    float *out = A.out + (size_t)b * 3 * plane;
    for (int base = 0; base < total; base += 64) {
        const int s = base + lane;
        const bool have = s < total;
        const int sr = have ? s / C : 0, sc = have ? s - sr * C : 0;
        const int oi = r0 + sr, oj = c0 + sc;
        const float px = A.sample_x[oj], py = A.sample_y[oi];
        float ar = init.x, ag = init.y, ab = init.z;
        for (int t = 0; t < n; ++t) {
            // the rasterizer's op sequence (common.h splat_sigma_h, exp_neg)
            const float4 G = s_geo[t];
            const float4 Cc = s_col[t];
            const float bl = s_blu[t];
            const float dy = G.y - py;
            const float cq = (Cc.x * dy) * dy;
            const float bdy = G.w * dy;
            const float dx = G.x - px;
            const float sg = fmaf(fmaf(G.z, dx, bdy), dx, cq);
            const float al = fminf(1.0f, Cc.y * __builtin_amdgcn_exp2f(sg * kNegLog2e));
            const bool ok = !(sg < 0.0f) && !(al < kAlphaMin);
            const float nr = fmaf(Cc.z, al, ar), ng = fmaf(Cc.w, al, ag), nb = fmaf(bl, al, ab);
            ar = ok ? nr : ar;
            ag = ok ? ng : ag;
            ab = ok ? nb : ab;
        }
        if (have) {
            float *o = out + (size_t)oi * (size_t)A.out_w + (size_t)oj;
            o[0] = clamp01_keep_nan(ar);
            o[plane] = clamp01_keep_nan(ag);
            o[2 * plane] = clamp01_keep_nan(ab);
        }
    }
}

// A partition of [0, count) into n consecutive, possibly empty ranges.
static bool partitions(const int *start, int n, unsigned count) {
    if (start[0] != 0 || start[n] != (int)count) return false;
    for (int t = 0; t < n; ++t)
        if (start[t + 1] < start[t]) return false;
    return true;
}

}  // namespace gsvc

using namespace gsvc;

extern "C" int gsvc_render_frames_resampled(
    int frames, const int *frame_offsets_host, const int *frame_offsets_dev, const float *xyz,
    int xyz_tanh, const float *cholesky, const float *cholesky_bound, const float *features,
    const float *rgb_w, const float *opacity, const float *background, unsigned img_height,
    unsigned img_width, int call_index, int density_hint, int *meta, void *workspace,
    size_t workspace_bytes, const float *sample_x_host, const float *sample_y_host,
    const int *col_start_host, const int *row_start_host, const float *sample_x_dev,
    const float *sample_y_dev, const int *col_start_dev, const int *row_start_dev, unsigned out_h,
    unsigned out_w, float *out, void *stream) {
    (void)density_hint;  // one composite, whatever the density
    if (frames < 1 || frames > 4096 || img_height == 0 || img_width == 0 || out_h == 0 || out_w == 0 ||
        out_h > (1u << 30) || out_w > (1u << 30))
        return set_error(GSVC_ERR_ARG, "render_frames_resampled: bad sizes");
    if (!frame_offsets_host || !frame_offsets_dev || !background || !meta || !out || !workspace ||
        !sample_x_host || !sample_y_host || !col_start_host || !row_start_host || !sample_x_dev ||
        !sample_y_dev || !col_start_dev || !row_start_dev)
        return set_error(GSVC_ERR_ARG, "render_frames_resampled: missing input");
    if (frame_offsets_host[0] != 0)
        return set_error(GSVC_ERR_ARG, "render_frames_resampled: frame offsets must start at 0");
    const int n = frame_offsets_host[frames];
    int max_n = 0;
    for (int b = 0; b < frames; ++b) {
        const int nb = frame_offsets_host[b + 1] - frame_offsets_host[b];
        if (nb < 0 || frame_offsets_host[b] < 0 || frame_offsets_host[b + 1] > n)
            return set_error(GSVC_ERR_ARG, "render_frames_resampled: bad frame offsets");
        max_n = nb > max_n ? nb : max_n;
    }
    if (n > 0 && (!xyz || !cholesky || !features))
        return set_error(GSVC_ERR_ARG, "render_frames_resampled: missing input");
    const int tbx = ceil_div((int)img_width, kTile), tby = ceil_div((int)img_height, kTile);
    const int ntiles = tbx * tby;
    // every output sample has exactly one owner tile: the kernel's only indices
    // into out and the sample tables come from these ranges
    if (!partitions(col_start_host, tbx, out_w) || !partitions(row_start_host, tby, out_h))
        return set_error(GSVC_ERR_ARG, "render_frames_resampled: the start tables do not partition "
                                       "the output's rows and columns");
    for (unsigned j = 0; j < out_w; ++j)
        if (!(sample_x_host[j] >= -1.0f && sample_x_host[j] <= (float)img_width))
            return set_error(GSVC_ERR_ARG, "render_frames_resampled: sample_x[%u] outside the frame", j);
    for (unsigned i = 0; i < out_h; ++i)
        if (!(sample_y_host[i] >= -1.0f && sample_y_host[i] <= (float)img_height))
            return set_error(GSVC_ERR_ARG, "render_frames_resampled: sample_y[%u] outside the frame", i);
    const FrameWs w = frame_ws((char *)workspace, n, ntiles, frames);
    if (workspace_bytes < w.bytes)
        return set_error(GSVC_ERR_WORKSPACE, "render_frames_resampled: workspace too small (%zu < %zu)",
                         workspace_bytes, w.bytes);
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = refuse_capture(s, "render_frames_resampled")) return rc;
    const FrameSlots f = frame_slots(w, ntiles, call_index);
    // record slabs at any frame count (a single frame projects as a batch of one)
    int rc = frame_project_launch(n, xyz, xyz_tanh, cholesky, cholesky_bound, features, rgb_w, opacity,
                                  img_height, img_width, w, f, nullptr, s, frames, frame_offsets_dev,
                                  max_n, nullptr, nullptr);
    if (rc) return rc;
    ResampleArgs A;
    A.tbx = tbx;
    A.tby = tby;
    A.ntiles = ntiles;
    A.frames = frames;
    A.out_w = (int)out_w;
    A.out_h = (int)out_h;
    A.sample_x = sample_x_dev;
    A.sample_y = sample_y_dev;
    A.col_start = col_start_dev;
    A.row_start = row_start_dev;
    A.m_dev = f.m_acc;
    A.meta_out = meta;
    A.bg = background;
    A.slab = w.slab;
    A.slab_ovf = w.ovf;
    A.slab_counts = f.counts;
    A.slab_counts_clear = f.counts_next;
    A.cull_xys = w.xys;
    A.cull_radii = w.radii;
    A.rec = w.rec;
    A.frame_off = frame_offsets_dev;
    A.counts_stride = f.counts_stride;
    A.m_stride = f.m_stride;
    A.slab_stride = slab_frame_f4(ntiles);
    A.out = out;
    hipLaunchKernelGGL(raster_resampled_kernel, dim3(ntiles * frames), dim3(64), 0, s, A);
    return check_launch("render_frames_resampled");
}
