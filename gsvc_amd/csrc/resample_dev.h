// The resampled composites' shared part (resample.hip, resample_aa.hip): the
// host checks and source-size projection of an entry that takes a view's four
// tables, and the device code every composite wave starts with -- the tile's
// bookkeeping, its ids sorted by tile_ids.h, their records gathered into LDS --
// and the rasterizer's op sequence at one sample position.
#pragma once

#include "frame.h"
#include "tile_ids.h"

namespace gsvc {

struct ResampleArgs {
    int tbx, ntiles, frames;
    int out_w, out_h;                  // the size the tables partition
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

// What a composite wave knows of its (frame, source tile) before it looks at
// the tile's output rectangle.
struct ResampleTile {
    int b, tile, n_all, m_val;
};

// The wave's frame and tile from its block index; clears the tile's counts of
// the next call and, from tile 0, writes the frame's meta.
__device__ __forceinline__ ResampleTile resample_tile_begin(const ResampleArgs &A) {
    const int lane = threadIdx.x & 63;
    ResampleTile T;
    T.tile = xcd_runs<16>(blockIdx.x, A.ntiles * A.frames);
    T.b = T.tile / A.ntiles;
    T.tile -= T.b * A.ntiles;
    const unsigned *counts = A.slab_counts + (size_t)T.b * A.counts_stride;
    unsigned *counts_clear = A.slab_counts_clear + (size_t)T.b * A.counts_stride;
    T.m_val = A.m_dev[(size_t)T.b * A.m_stride];
    T.n_all = (int)__builtin_amdgcn_readfirstlane(counts[T.tile]);
    if (lane == 0) {
        counts_clear[T.tile] = 0u;  // the next call's counts
        if (T.tile == 0) {
            A.meta_out[(size_t)T.b * A.m_stride] = T.m_val;
            A.meta_out[(size_t)T.b * A.m_stride + 1] = 0;
        }
    }
    return T;
}

// The tile's entry list staged in LDS (kTilePix slots each; s_geo holds the
// sort's bitmap before staging): returns its length, wave-uniform, and the
// value a sample starts from (rasterize_sum.py:121-127: a frame without
// intersections is the background, and has no entries).
__device__ __forceinline__ int resample_tile_stage(const ResampleArgs &A, const ResampleTile &T,
                                                   float4 *s_geo, float4 *s_col, float *s_blu,
                                                   int *s_ids, float3 &init) {
    const int lane = threadIdx.x & 63;
    init = make_float3(0.f, 0.f, 0.f);
    if (T.m_val < 1) {
        init = make_float3(A.bg[0], A.bg[1], A.bg[2]);
        return 0;
    }
    const float4 *slab = A.slab + T.b * A.slab_stride;
    const int *ovf = A.slab_ovf + (size_t)T.b * kOvfSlots * (size_t)A.ntiles;
    // the native composite's list: the slab's ids (slots past 256 from the
    // overflow ids) sorted, or past kCarryCap the first 256 by the bbox
    // rebuild over the frame's splats
    SegIds seg;
    seg.ids = nullptr;
    seg.recs = slab_rec(slab, A.ntiles, T.tile, kHeadSlots) - 3 * kHeadSlots;
    seg.head = slab_rec(slab, A.ntiles, T.tile, 0);
    seg.ovf = ovf + (size_t)T.tile * kOvfSlots;
    int n = T.n_all > seg.cap()
                ? wave_brute_ids(A.cull_xys, A.cull_radii, A.frame_off[T.b], A.frame_off[T.b + 1], A.tbx,
                                 A.tby, T.tile, s_ids)
                : wave_sorted_tile_ids(seg, T.n_all, s_ids, reinterpret_cast<unsigned *>(s_geo));
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
    return n;
}

// The staged list at (px, py), from ``init``: the rasterizer's op sequence
// (common.h splat_sigma_h, exp_neg), every lane reading a wave-uniform address.
__device__ __forceinline__ void resample_composite(const float4 *s_geo, const float4 *s_col,
                                                   const float *s_blu, int n, float px, float py,
                                                   const float3 &init, float &ar, float &ag, float &ab) {
    ar = init.x, ag = init.y, ab = init.z;
    for (int t = 0; t < n; ++t) {
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
}

// A partition of [0, count) into n consecutive, possibly empty ranges.
static inline bool partitions(const int *start, int n, unsigned count) {
    if (start[0] != 0 || start[n] != (int)count) return false;
    for (int t = 0; t < n; ++t)
        if (start[t + 1] < start[t]) return false;
    return true;
}

// The host side both entries share, ``name`` the entry's for the messages.
// resample_check: every check of include/gsvc_amd.h on the sizes, the buffers,
// the frame offsets, the workspace and the four tables (which partition
// out_h x out_w); nothing is launched.  0, or the status to return.
static inline int resample_check(
    const char *name, int frames, const int *frame_offsets_host, const int *frame_offsets_dev,
    const float *xyz, const float *cholesky, const float *features, const float *background,
    unsigned img_height, unsigned img_width, const int *meta, const void *workspace,
    size_t workspace_bytes, const float *sample_x_host, const float *sample_y_host,
    const int *col_start_host, const int *row_start_host, const float *sample_x_dev,
    const float *sample_y_dev, const int *col_start_dev, const int *row_start_dev, unsigned out_h,
    unsigned out_w, const float *out, hipStream_t s) {
    if (frames < 1 || frames > 4096 || img_height == 0 || img_width == 0 || out_h == 0 || out_w == 0 ||
        out_h > (1u << 30) || out_w > (1u << 30))
        return set_error(GSVC_ERR_ARG, "%s: bad sizes", name);
    if (!frame_offsets_host || !frame_offsets_dev || !background || !meta || !out || !workspace ||
        !sample_x_host || !sample_y_host || !col_start_host || !row_start_host || !sample_x_dev ||
        !sample_y_dev || !col_start_dev || !row_start_dev)
        return set_error(GSVC_ERR_ARG, "%s: missing input", name);
    if (frame_offsets_host[0] != 0)
        return set_error(GSVC_ERR_ARG, "%s: frame offsets must start at 0", name);
    const int n = frame_offsets_host[frames];
    for (int b = 0; b < frames; ++b) {
        const int nb = frame_offsets_host[b + 1] - frame_offsets_host[b];
        if (nb < 0 || frame_offsets_host[b] < 0 || frame_offsets_host[b + 1] > n)
            return set_error(GSVC_ERR_ARG, "%s: bad frame offsets", name);
    }
    if (n > 0 && (!xyz || !cholesky || !features))
        return set_error(GSVC_ERR_ARG, "%s: missing input", name);
    const int tbx = ceil_div((int)img_width, kTile), tby = ceil_div((int)img_height, kTile);
    const int ntiles = tbx * tby;
    // every sample has exactly one owner tile: the kernels' only indices into
    // the sample tables (and, point-sampled, into out) come from these ranges
    if (!partitions(col_start_host, tbx, out_w) || !partitions(row_start_host, tby, out_h))
        return set_error(GSVC_ERR_ARG, "%s: the start tables do not partition the output's rows and "
                                       "columns", name);
    for (unsigned j = 0; j < out_w; ++j)
        if (!(sample_x_host[j] >= -1.0f && sample_x_host[j] <= (float)img_width))
            return set_error(GSVC_ERR_ARG, "%s: sample_x[%u] outside the frame", name, j);
    for (unsigned i = 0; i < out_h; ++i)
        if (!(sample_y_host[i] >= -1.0f && sample_y_host[i] <= (float)img_height))
            return set_error(GSVC_ERR_ARG, "%s: sample_y[%u] outside the frame", name, i);
    const FrameWs w = frame_ws((char *)const_cast<void *>(workspace), n, ntiles, frames);
    if (workspace_bytes < w.bytes)
        return set_error(GSVC_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu)", name, workspace_bytes,
                         w.bytes);
    return refuse_capture(s, name);
}

// resample_project: after resample_check, the projection at the source size
// into the shared workspace (record slabs at any frame count: a single frame
// projects as a batch of one), then A filled for the composite.
static inline int resample_project(
    int frames, const int *frame_offsets_host, const int *frame_offsets_dev, const float *xyz,
    int xyz_tanh, const float *cholesky, const float *cholesky_bound, const float *features,
    const float *rgb_w, const float *opacity, const float *background, unsigned img_height,
    unsigned img_width, int call_index, int *meta, void *workspace, const float *sample_x_dev,
    const float *sample_y_dev, const int *col_start_dev, const int *row_start_dev, unsigned out_h,
    unsigned out_w, float *out, hipStream_t s, ResampleArgs &A) {
    const int n = frame_offsets_host[frames];
    int max_n = 0;
    for (int b = 0; b < frames; ++b) {
        const int nb = frame_offsets_host[b + 1] - frame_offsets_host[b];
        max_n = nb > max_n ? nb : max_n;
    }
    const int tbx = ceil_div((int)img_width, kTile), tby = ceil_div((int)img_height, kTile);
    const int ntiles = tbx * tby;
    const FrameWs w = frame_ws((char *)workspace, n, ntiles, frames);
    const FrameSlots f = frame_slots(w, ntiles, call_index);
    const int rc = frame_project_launch(n, xyz, xyz_tanh, cholesky, cholesky_bound, features, rgb_w,
                                        opacity, img_height, img_width, w, f, nullptr, s, frames,
                                        frame_offsets_dev, max_n, nullptr, nullptr);
    if (rc) return rc;
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
    return 0;
}

}  // namespace gsvc
