// Batched frame render through a view with a box prefilter (gfx950): every
// output pixel the mean of ky x kx point samples of the view's FINE view, the
// sub-samples evaluated and reduced by the composite itself (include/gsvc_amd.h
// gsvc_render_frames_filtered: the rule and its summation order; DESIGN.md
// §13h).  The fine image never exists: a wave stores one value per output
// pixel and channel, 1 / (ky kx) of the fine view's traffic.
//
// Three kernels: the frame projection of frame.hip at the SOURCE size, as
// gsvc_render_frames_resampled (resample_dev.h), then
//   raster_filtered_kernel  one wave per (frame, source tile), the tile's list
//                           sorted and staged as in resample.hip.  The tile
//                           owns the fine rectangle rows [row_start[ty],
//                           row_start[ty + 1]) x columns [col_start[tx],
//                           col_start[tx + 1]) and touches the output pixels
//                           that hold one of those samples.  Lane = sub-sample:
//                           groups of ky kx consecutive lanes, one output pixel
//                           each, floor(64 / (ky kx)) pixels of the touched
//                           range per trip; a lane whose sub-sample lies
//                           outside the rectangle (another tile's) contributes
//                           +0.0f.  The clamped values go through LDS and the
//                           group's lane c < 3 adds channel c's in row-major
//                           order from +0.0f: for a pixel wholly inside the
//                           tile that is the rule's sum, divided and stored to
//                           out; for a pixel that straddles a tile edge it is
//                           the rule's part of this tile, stored to
//                           parts[frame][slot][3][out_h][out_w].
//   filter_seams_kernel     one thread per output pixel: straddlers, found
//                           from the tables as the first kernel finds them, add
//                           their 2 or 4 parts in slot order, divide and store
//                           (not launched for a view without a straddler, such
//                           as an integer downscale by a divisor of 16).
// No atomics and no zero fill: a straddler's slots are exactly the tiles that
// own one of its sub-samples, each written by that tile's wave in this call
// (the <= 2 tiles per axis condition, checked on the host, makes them 2 x 2).
#include "resample_dev.h"

namespace gsvc {

struct FilterArgs {
    ResampleArgs R;    // the fine view's tables and size; R.out is the final image
    int ky, kx;
    int out_h, out_w;  // the final size: R.out_h = ky out_h, R.out_w = kx out_w
    float *parts;
};

// (10 KB of LDS per wave, as raster_resampled_kernel: 16 waves per CU)
__global__ __launch_bounds__(64) void raster_filtered_kernel(FilterArgs F) {
    __shared__ float4 s_geo[kTilePix];  // x, y, a/2, b (the sort's bitmap before staging)
    __shared__ float4 s_col[kTilePix];  // c/2, opacity, r, g
    __shared__ float s_blu[kTilePix];   // b
    __shared__ __align__(16) int s_ids[kTilePix];  // the tile's sorted ids; after staging s_red
    static_assert(sizeof(float4) * kTilePix >= sizeof(unsigned) * kSortWords, "bitmap in s_geo");
    static_assert(sizeof(int) * kTilePix >= sizeof(float) * 3 * 64, "s_red in s_ids");
    const ResampleArgs &A = F.R;
    const int lane = threadIdx.x & 63;
    const ResampleTile T = resample_tile_begin(A);
    const int ty = T.tile / A.tbx, tx = T.tile - ty * A.tbx;
    const int fr0 = A.row_start[ty], fr1 = A.row_start[ty + 1];
    const int fc0 = A.col_start[tx], fc1 = A.col_start[tx + 1];
    if (fr1 <= fr0 || fc1 <= fc0) return;  // the tile owns no sub-sample (wave-uniform)
    float3 init;
    const int n = resample_tile_stage(A, T, s_geo, s_col, s_blu, s_ids, init);
    // a trip's clamped sub-samples, per channel, where the ids were (dead once staged)
    float(*s_red)[64] = reinterpret_cast<float(*)[64]>(s_ids);
    const int ky = F.ky, kx = F.kx, g = ky * kx, per_trip = 64 / g;
    // the output pixels that hold one of the tile's sub-samples
    const int pi0 = fr0 / ky, pj0 = fc0 / kx;
    const int PC = (fc1 - 1) / kx + 1 - pj0, pixels = ((fr1 - 1) / ky + 1 - pi0) * PC;
    const int grp = lane / g, sub = lane - grp * g;
    const int sa = sub / kx, sb = sub - sa * kx;
    const size_t plane = (size_t)F.out_w * (size_t)F.out_h;
    float *out = A.out + (size_t)T.b * 3 * plane;
    float *parts = F.parts + (size_t)T.b * 12 * plane;
    const float fg = (float)g;
    for (int base = 0; base < pixels; base += per_trip) {
        const int p = base + grp;
        const bool have = grp < per_trip && p < pixels;
        const int pr = have ? p / PC : 0, pc = have ? p - pr * PC : 0;
        const int oi = pi0 + pr, oj = pj0 + pc;
        const int fi = oi * ky + sa, fj = oj * kx + sb;
        const bool mine = have && fi >= fr0 && fi < fr1 && fj >= fc0 && fj < fc1;
        const float px = A.sample_x[mine ? fj : fc0], py = A.sample_y[mine ? fi : fr0];
        float ar, ag, ab;
        resample_composite(s_geo, s_col, s_blu, n, px, py, init, ar, ag, ab);
        s_red[0][lane] = mine ? clamp01_keep_nan(ar) : 0.0f;
        s_red[1][lane] = mine ? clamp01_keep_nan(ag) : 0.0f;
        s_red[2][lane] = mine ? clamp01_keep_nan(ab) : 0.0f;
        wave_lds_sync();
        if (have) {
            // where the pixel's sub-sample rows and columns leave the tile
            const bool rlo = oi * ky < fr0, rhi = oi * ky + ky > fr1;
            const bool clo = oj * kx < fc0, chi = oj * kx + kx > fc1;
            const bool whole = !(rlo || rhi || clo || chi);
            const int slot = 2 * (rlo ? 1 : 0) + (clo ? 1 : 0);
            const size_t at = (size_t)oi * (size_t)F.out_w + (size_t)oj;
            for (int c = sub; c < 3; c += g) {  // (g >= 3: lanes 0..2 of the group, one channel each)
                const float *q = &s_red[c][grp * g];
                float acc = 0.0f;  // then row-major (a, b), one add after the other
                if ((g & 3) == 0) {  // (16-byte aligned: grp * g is a multiple of 4)
                    for (int t = 0; t < g; t += 4) {
                        const float4 v = *reinterpret_cast<const float4 *>(q + t);
                        acc = ((acc + v.x) + v.y) + v.z;
                        acc += v.w;
                    }
                } else {
                    for (int t = 0; t < g; ++t) acc += q[t];
                }
                if (whole)
                    out[(size_t)c * plane + at] = acc / fg;
                else
                    parts[(size_t)(3 * slot + c) * plane + at] = acc;
            }
        }
        wave_lds_sync();  // the next trip overwrites s_red
    }
}

// The tile whose range [start[t], start[t + 1]) holds r, for 0 <= r < start[tiles].
__host__ __device__ __forceinline__ int owner_tile(const int *start, int tiles, int r) {
    int lo = 0, hi = tiles - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (start[mid + 1] > r)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void filter_seams_kernel(FilterArgs F) {
    const ResampleArgs &A = F.R;
    const size_t plane = (size_t)F.out_w * (size_t)F.out_h;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= plane * (size_t)A.frames) return;
    const size_t b = idx / plane, at = idx - b * plane;
    const int oi = (int)(at / (size_t)F.out_w), oj = (int)(at - (size_t)oi * (size_t)F.out_w);
    const int rf = oi * F.ky, cf = oj * F.kx;
    const bool rs = A.row_start[owner_tile(A.row_start, A.tby, rf) + 1] < rf + F.ky;
    const bool cs = A.col_start[owner_tile(A.col_start, A.tbx, cf) + 1] < cf + F.kx;
    if (!rs && !cs) return;  // wholly inside one tile: stored by that tile's wave
    const float *parts = F.parts + b * 12 * plane + at;
    float *out = A.out + b * 3 * plane + at;
    const float fg = (float)(F.ky * F.kx);
    for (int c = 0; c < 3; ++c) {
        float acc = parts[(size_t)c * plane];
        if (cs) acc += parts[(size_t)(3 + c) * plane];
        if (rs) acc += parts[(size_t)(6 + c) * plane];
        if (rs && cs) acc += parts[(size_t)(9 + c) * plane];
        out[(size_t)c * plane] = acc / fg;
    }
}

// Every output pixel's k sub-samples of one axis lie on the first one's tile
// or the next; ``seams`` counts the pixels that lie on both.
static bool at_most_two_tiles(const int *start, int tiles, unsigned out, unsigned k, unsigned &seams) {
    seams = 0;
    for (unsigned i = 0; i < out; ++i) {
        const int d = owner_tile(start, tiles, (int)(i * k + k - 1)) - owner_tile(start, tiles, (int)(i * k));
        if (d > 1) return false;
        seams += (unsigned)d;
    }
    return true;
}

}  // namespace gsvc

using namespace gsvc;

extern "C" int gsvc_render_frames_filtered(
    int frames, const int *frame_offsets_host, const int *frame_offsets_dev, const float *xyz,
    int xyz_tanh, const float *cholesky, const float *cholesky_bound, const float *features,
    const float *rgb_w, const float *opacity, const float *background, unsigned img_height,
    unsigned img_width, int call_index, int density_hint, int *meta, void *workspace,
    size_t workspace_bytes, const float *sample_x_host, const float *sample_y_host,
    const int *col_start_host, const int *row_start_host, const float *sample_x_dev,
    const float *sample_y_dev, const int *col_start_dev, const int *row_start_dev, unsigned ky,
    unsigned kx, unsigned out_h, unsigned out_w, float *parts, size_t parts_bytes, float *out,
    void *stream) {
    (void)density_hint;  // one composite, whatever the density
    static const char *const kName = "render_frames_filtered";
    if (ky == 0 || kx == 0 || ky > 64 || kx > 64 || ky * kx > 64)
        return set_error(GSVC_ERR_ARG, "%s: bad sizes: ky, kx >= 1 and ky kx <= 64, not %u x %u", kName, ky,
                         kx);
    if (out_h == 0 || out_w == 0 || out_h > (1u << 30) / ky || out_w > (1u << 30) / kx)
        return set_error(GSVC_ERR_ARG, "%s: bad sizes", kName);
    const unsigned fine_h = ky * out_h, fine_w = kx * out_w;
    hipStream_t s = (hipStream_t)stream;
    int rc = resample_check(kName, frames, frame_offsets_host, frame_offsets_dev, xyz, cholesky, features,
                            background, img_height, img_width, meta, workspace, workspace_bytes,
                            sample_x_host, sample_y_host, col_start_host, row_start_host, sample_x_dev,
                            sample_y_dev, col_start_dev, row_start_dev, fine_h, fine_w, out, s);
    if (rc) return rc;
    const int tbx = ceil_div((int)img_width, kTile), tby = ceil_div((int)img_height, kTile);
    unsigned seam_rows = 0, seam_cols = 0;
    if (!at_most_two_tiles(row_start_host, tby, out_h, ky, seam_rows) ||
        !at_most_two_tiles(col_start_host, tbx, out_w, kx, seam_cols))
        return set_error(GSVC_ERR_ARG, "%s: an output pixel's sub-samples lie on more than two tiles along "
                                       "an axis", kName);
    const size_t pixels = (size_t)frames * (size_t)out_h * (size_t)out_w;
    if (!parts) return set_error(GSVC_ERR_ARG, "%s: missing input", kName);
    if (parts_bytes / (12 * sizeof(float)) < pixels)
        return set_error(GSVC_ERR_ARG, "%s: parts holds %zu bytes, %zu floats are needed", kName,
                         parts_bytes, 12 * pixels);
    const size_t seam_blocks = (pixels + 255) / 256;
    if (seam_blocks > 0x7fffffffull) return set_error(GSVC_ERR_ARG, "%s: bad sizes", kName);
    FilterArgs F;
    rc = resample_project(frames, frame_offsets_host, frame_offsets_dev, xyz, xyz_tanh, cholesky,
                          cholesky_bound, features, rgb_w, opacity, background, img_height, img_width,
                          call_index, meta, workspace, sample_x_dev, sample_y_dev, col_start_dev,
                          row_start_dev, fine_h, fine_w, out, s, F.R);
    if (rc) return rc;
    F.ky = (int)ky;
    F.kx = (int)kx;
    F.out_h = (int)out_h;
    F.out_w = (int)out_w;
    F.parts = parts;
    hipLaunchKernelGGL(raster_filtered_kernel, dim3(F.R.ntiles * frames), dim3(64), 0, s, F);
    rc = check_launch(kName);
    if (rc || (seam_rows == 0 && seam_cols == 0)) return rc;  // (no straddler: every pixel is stored)
    hipLaunchKernelGGL(filter_seams_kernel, dim3((unsigned)seam_blocks), dim3(256), 0, s, F);
    return check_launch(kName);
}
