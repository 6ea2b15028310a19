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
// The host checks, the projection call and the wave's staging and op sequence
// are resample_dev.h's, shared with the filtered composite (resample_aa.hip).
#include "resample_dev.h"

namespace gsvc {

// (10 KB of LDS per wave: 16 waves per CU, 4 per SIMD)
__global__ __launch_bounds__(64) void raster_resampled_kernel(ResampleArgs A) {
    __shared__ float4 s_geo[kTilePix];  // x, y, a/2, b (the sort's bitmap before staging)
    __shared__ float4 s_col[kTilePix];  // c/2, opacity, r, g
    __shared__ float s_blu[kTilePix];   // b
    __shared__ int s_ids[kTilePix];     // the tile's sorted ids
    static_assert(sizeof(float4) * kTilePix >= sizeof(unsigned) * kSortWords, "bitmap in s_geo");
    const int lane = threadIdx.x & 63;
    const ResampleTile T = resample_tile_begin(A);
    const int b = T.b;
    const int ty = T.tile / A.tbx, tx = T.tile - ty * A.tbx;
    const int r0 = A.row_start[ty], r1 = A.row_start[ty + 1];
    const int c0 = A.col_start[tx], c1 = A.col_start[tx + 1];
    const int C = c1 - c0, total = (r1 - r0) * C;
    if (total <= 0) return;  // the tile owns no output sample (wave-uniform)
    float3 init;
    const int n = resample_tile_stage(A, T, s_geo, s_col, s_blu, s_ids, init);
    const size_t plane = (size_t)A.out_w * (size_t)A.out_h;
    float *out = A.out + (size_t)b * 3 * plane;
    for (int base = 0; base < total; base += 64) {
        const int s = base + lane;
        const bool have = s < total;
        const int sr = have ? s / C : 0, sc = have ? s - sr * C : 0;
        const int oi = r0 + sr, oj = c0 + sc;
        const float px = A.sample_x[oj], py = A.sample_y[oi];
        float ar, ag, ab;
        resample_composite(s_geo, s_col, s_blu, n, px, py, init, ar, ag, ab);
        if (have) {
            float *o = out + (size_t)oi * (size_t)A.out_w + (size_t)oj;
            o[0] = clamp01_keep_nan(ar);
            o[plane] = clamp01_keep_nan(ag);
            o[2 * plane] = clamp01_keep_nan(ab);
        }
    }
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
    hipStream_t s = (hipStream_t)stream;
    static const char *const kName = "render_frames_resampled";
    int rc = resample_check(kName, frames, frame_offsets_host, frame_offsets_dev, xyz, cholesky, features,
                            background, img_height, img_width, meta, workspace, workspace_bytes,
                            sample_x_host, sample_y_host, col_start_host, row_start_host, sample_x_dev,
                            sample_y_dev, col_start_dev, row_start_dev, out_h, out_w, out, s);
    if (rc) return rc;
    ResampleArgs A;
    rc = resample_project(frames, frame_offsets_host, frame_offsets_dev, xyz, xyz_tanh, cholesky,
                          cholesky_bound, features, rgb_w, opacity, background, img_height, img_width,
                          call_index, meta, workspace, sample_x_dev, sample_y_dev, col_start_dev,
                          row_start_dev, out_h, out_w, out, s, A);
    if (rc) return rc;
    hipLaunchKernelGGL(raster_resampled_kernel, dim3(A.ntiles * frames), dim3(64), 0, s, A);
    return check_launch(kName);
}
